"""Drop-in for the reference ``polyffusion/inference_sdf.py`` on the denoising path.

Kept from the reference: the flag names (``inference_sdf.py:404-507``, typed properly - the
reference leaves ``--ddim_steps``/``--ddim_eta`` as strings), the
``params.yaml`` discovery rule (:518-532), model assembly (:536-557), checkpoint loading for the
legacy ``.pt`` format (:702-716), ``Experiments.predict/generate/inpaint`` incl. the
autoregressive 4-bar inpainting schedule (:202-303), ``get_autoreg_data`` (:121-129),
``dummy_cond_input`` (:60-72) and ``get_mask`` (:132-193).

Not rebuilt (out of the hot-path scope): dataset / MIDI readers, chord
extraction, Polydis comparison.  Conditions therefore come from ``--from_song_npz`` (a quantised song in the reference's data-dictionary format,
segmented by ``polyffusion_amd.datasample``), from ``--cond_npz`` (arrays
``chord`` [B,32,36] and/or ``prmat`` [B,128,128], optional ``prmat2c`` for inpainting) or from the
seeded synthetic generator (``--synthetic``); the result is written as ``.mid`` (polyffusion_amd.midi) and ``.npy`` ([B,2,128,128] piano
roll, or [2B,2,64,128] half-segments for ``--autoreg``; ``--joint``, an extension, denoises the 2B-1 half-overlapping windows of a song
in one reverse loop and writes [B,2,128,128]; ``--edit``, an extension, changes the condition song itself by exact DDIM inversion -
``Experiments.edit`` - instead of generating from noise; ``--morph``, an extension, writes the frames of a path between the condition
song and a second one - ``Experiments.morph`` - as [K,B,2,128,128]).  ``--synthetic_weights`` replaces the
checkpoint by the deterministic weight generator (no trained weights ship with the reference).
"""
from __future__ import annotations

import json
import math
import os
import random
from argparse import ArgumentParser
from datetime import datetime
from typing import Optional

import numpy as np
import torch

from . import _lib, datasample, midi, synth
from . import chordrec as pfchordrec
from . import rollmatch as pfrollmatch
from . import score as pfscore
from .model_sdf import ChordEncoder, Polyffusion_SDF, TextureEncoder
from .params import Params, find_params, load_params, preset
from .sampler import (DPM_STEER_REFUSAL, GUIDANCE_ORDERS, MORPH_CONDS, MORPH_EASES, DDIMSampler, DiffusionSampler, DPMSolverSampler, DualScale, SDFSampler,
                      Steering, SteeringRecord, X0Threshold, guidance_interval_from_fractions)
from .unet import LatentDiffusion, UNetModel


POLYDIS_MODEL_PATH = "pretrained/polydis/model_master_final.pt"   # ref:polydis_aftertouch.py:6


def _dev():
    return torch.device("cuda", torch.cuda.current_device())


def dummy_cond_input(length, params):
    h, w = params.img_h, params.img_w
    prmat2c = torch.zeros([length, 2, h, w], device=_dev())
    chord = torch.zeros([length, params.chd_n_step, params.chd_input_dim], device=_dev()) if "chord" in params.cond_type else None
    prmat = torch.zeros([length, h, w], device=_dev())
    pnotree = torch.zeros([length, h, 20, 6], dtype=torch.int64, device=_dev())     # ref:inference_sdf.py:64
    return prmat2c, pnotree, chord, prmat


def get_blurry_image(img: torch.Tensor, ratio: float = 1 / 8) -> torch.Tensor:
    """``utils.py:552-567``: bicubic down by ``ratio``, nearest back up, clipped to [0, 1] - the ``cond_concat`` image of the
    ``concat_blurry`` variant (``inference_sdf.py:797-803``).  Preparation of an input, not part of the step loop: torch ops."""
    small = torch.nn.functional.interpolate(img, scale_factor=ratio, mode="bicubic")
    return torch.nn.functional.interpolate(small, scale_factor=1 / ratio, mode="nearest").clip(0, 1)


def get_autoreg_data(data: torch.Tensor, split_dim: int = 1) -> torch.Tensor:
    """(second half of item i, first half of item i+1): the half-shifted stream for odd runs."""
    steps = data.shape[split_dim]
    half_1, half_2 = data.split(steps // 2, dim=split_dim)
    return torch.cat((half_2, half_1.roll(-1, dims=0)), dim=split_dim)


def get_mask(orig: torch.Tensor, inpaint_type: str, bar_list=None) -> torch.Tensor:
    """Inpainting masks (1 = keep the original).  Vectorised restatement of the reference's row loops."""
    B = orig.shape[0]
    if inpaint_type == "remaining":
        return orig.clone()
    if inpaint_type in ("below", "above"):
        onset = orig[:, 0]
        steps, pitches = onset.shape[1], onset.shape[2]
        flat = onset.reshape(B * steps, pitches)
        if inpaint_type == "below":
            edge = flat.argmax(dim=1)            # lowest onset per step; 0 doubles as "no onset" (reference quirk)
            sentinel = 0
        else:
            edge = (pitches - 1) - flat.flip(1).argmax(dim=1)
            sentinel = pitches - 1               # "no onset" for the top edge
        nz = edge.nonzero()                      # the reference tests `!= 0` for BOTH types (:145,:167)
        if nz.numel() == 0:
            raise IndexError("get_mask: no usable onsets in the original (the reference fails here too)")
        first = int(nz[0, 0])
        edge[:first] = edge[first]
        # sequential rule of the reference: a "no onset" step copies the previous step, step 0 wraps to the last
        if int(edge[0]) == sentinel:
            edge[0] = edge[-1]
        empty = edge == sentinel
        empty[0] = False
        idx = torch.arange(B * steps, device=orig.device)
        last = torch.where(empty, torch.full_like(idx, -1), idx).cummax(0).values
        edge = edge[last]
        cols = torch.arange(pitches, device=orig.device)[None, :]
        m = (cols >= edge[:, None]) if inpaint_type == "below" else (cols <= edge[:, None])
        return m.to(orig.dtype).reshape(B, 1, steps, pitches).expand(-1, 2, -1, -1).contiguous()
    if inpaint_type == "bars":
        if bar_list is None:
            raise ValueError("get_mask('bars') needs bar_list (the reference prompts on stdin)")
        mask = torch.ones_like(orig)
        for bar in bar_list:
            mask[:, :, bar * 16: bar * 16 + 16, :] = 0
        return mask
    raise NotImplementedError(inpaint_type)


class Experiments:
    """``inference_sdf.py:196-400``.  ``t_idx`` replaces the reference's read of the module-global
    ``args`` (ddim_steps-1 or n_steps-1); ``noise`` lets tests inject the start noise."""

    def __init__(self, model_label, params, sampler: DiffusionSampler, t_idx: Optional[int] = None, repaint_n: int = 1):
        self.model_label = model_label
        self.params = params if isinstance(params, Params) else Params(params)
        self.sampler = sampler
        if t_idx is None:
            t_idx = (len(sampler.time_steps) - 1) if isinstance(sampler, (DDIMSampler, DPMSolverSampler)) else self.params.n_steps - 1
        self.t_idx = int(t_idx)
        self.repaint_n = int(repaint_n)

    @torch.no_grad()
    def predict(self, cond: torch.Tensor, cond_mid: Optional[torch.Tensor] = None, uncond_scale=1.0, autoreg=False,
                orig=None, mask=None, cond_concat=None, noise: Optional[torch.Tensor] = None, joint: bool = False, blend: str = "mean"):
        """``joint``: the one-song form of ``predict_joint`` - all 2B-1 half-overlapping windows in one reverse loop; returns ``[B, C, H, W]``."""
        if joint:
            if autoreg:
                raise ValueError("predict: joint and autoreg are two ways to join the segments of a song: choose one")
            one = lambda v: None if v is None else v.unsqueeze(0)
            return self.predict_joint(one(cond), one(cond_mid), uncond_scale, one(orig), one(mask), one(cond_concat), one(noise), blend)[0]
        p, dev = self.params, cond.device
        B = cond.shape[0]
        shape = [B, p.out_channels, p.img_h, p.img_w]
        uncond_cond = -torch.ones([B, 1, p.d_cond], device=dev)
        if orig is None or mask is None:
            orig, mask = torch.zeros(shape, device=dev), torch.zeros(shape, device=dev)
        if noise is None:
            noise = self.sampler.randn(shape, dev)
        t_idx = self.t_idx
        kw = dict(uncond_scale=uncond_scale, cond_concat=cond_concat, repaint_n=self.repaint_n)
        if not autoreg:
            xt = self.sampler.q_sample(orig, t_idx, noise)
            return self.sampler.paint(xt, cond, t_idx, orig=orig, mask=mask, orig_noise=noise, uncond_cond=uncond_cond, **kw)
        assert cond_mid is not None
        half = p.img_h // 2
        orig, mask = orig.clone(), mask.clone()  # edited in place below, like the reference's views
        orig_mid, mask_mid, noise_mid = (get_autoreg_data(v, split_dim=2) for v in (orig, mask, noise))
        uc = uncond_cond[0:1]
        gen, new_half = [], None
        for idx in range(B * 2 - 1):  # inpaint a 4-bar half each time
            src = (cond_mid, orig_mid, mask_mid, noise_mid) if idx % 2 == 1 else (cond, orig, mask, noise)
            c_s, o_s, m_s, n_s = (v[idx // 2: idx // 2 + 1] for v in src)
            if idx != 0:
                o_s[:, :, 0:half, :] = new_half
                m_s[:, :, 0:half, :] = 1
            xt = self.sampler.q_sample(o_s, t_idx, n_s)
            x0 = self.sampler.paint(xt, c_s, t_idx, orig=o_s, mask=m_s, orig_noise=n_s, uncond_cond=uc, **kw)
            if idx == 0:
                gen.append(x0[:, :, 0:half, :])
            new_half = x0[:, :, half:, :]
            gen.append(new_half)
        gen = torch.cat(gen, dim=0)
        assert gen.shape[0] == B * 2
        return gen

    @torch.no_grad()
    def predict_songs(self, cond: torch.Tensor, cond_mid: torch.Tensor, uncond_scale=1.0, orig=None, mask=None,
                      cond_concat=None, noise: Optional[torch.Tensor] = None):
        """``predict(autoreg=True)`` (``inference_sdf.py:227-283``) batched ACROSS songs - BASELINE config 5.

        ``cond`` / ``cond_mid`` are ``[S, B, n_cond, d_cond]`` (S songs of B 8-bar segments); ``orig`` / ``mask`` / ``noise``,
        when given, ``[S, B, C, H, W]``.  The 2B-1 runs stay sequential within a song (run r needs the half that run r-1
        produced) but run r of all S songs is one batch of S images, so the denoiser sees batch S instead of batch 1.
        Song s gets exactly what ``predict(cond[s], cond_mid[s], autoreg=True, ...)`` computes when both are fed the same
        noise.  With the on-device generator the draws are keyed by (seed, draw counter, global song index): ranks that
        shard the songs (``sample_offset`` = first song of the rank) reproduce the unsharded run.
        Returns ``[S, 2B, C, H/2, W]``."""
        p, dev = self.params, cond.device
        S, B = cond.shape[0], cond.shape[1]
        shape = [S, B, p.out_channels, p.img_h, p.img_w]
        half = p.img_h // 2
        if cond_concat is not None:
            # the reference hands its WHOLE [B, ...] cond_concat to every batch-1 run (inference_sdf.py:259-270), which torch.cat
            # only accepts for B == 1: the concat_blurry variant can run autoregressively on one-segment songs only
            if cond_concat.dim() != 5 or cond_concat.shape[0] != S or cond_concat.shape[1] != B:
                raise RuntimeError(f"predict_songs: cond_concat must be [S, B, C, H, W] = [{S}, {B}, ...], got {tuple(cond_concat.shape)}")
            if B != 1:
                raise RuntimeError(f"Sizes of tensors must match except in dimension 1. Expected size 1 but got size {B} for tensor number 1 "
                                   "in the list. (cond_concat of a multi-segment song under --autoreg, as in the reference)")
            cond_concat = cond_concat[:, 0].contiguous()
        if orig is None or mask is None:
            orig, mask = torch.zeros(shape, device=dev), torch.zeros(shape, device=dev)
        else:
            orig, mask = orig.clone().float(), mask.clone().float()   # edited in place below
        if noise is None:
            noise = self.sampler.randn(shape, dev)
        # half-shifted streams per song: get_autoreg_data rolls along dim 0, so the segment axis goes there
        mid = lambda v: get_autoreg_data(v.transpose(0, 1), split_dim=3).transpose(0, 1)
        orig_mid, mask_mid, noise_mid = mid(orig), mid(mask), mid(noise)
        uc = -torch.ones([S, 1, p.d_cond], device=dev)
        kw = dict(uncond_scale=uncond_scale, uncond_cond=uc, cond_concat=cond_concat, repaint_n=self.repaint_n)
        gen, new_half = [], None
        for idx in range(B * 2 - 1):
            src = (cond_mid, orig_mid, mask_mid, noise_mid) if idx % 2 == 1 else (cond, orig, mask, noise)
            c_s, o_s, m_s, n_s = (v[:, idx // 2] for v in src)
            if idx != 0:
                o_s[:, :, 0:half, :] = new_half
                m_s[:, :, 0:half, :] = 1
            c_s, o_s, m_s, n_s = (v.contiguous() for v in (c_s, o_s, m_s, n_s))
            xt = self.sampler.q_sample(o_s, self.t_idx, n_s)
            x0 = self.sampler.paint(xt, c_s, self.t_idx, orig=o_s, mask=m_s, orig_noise=n_s, **kw)
            if idx == 0:
                gen.append(x0[:, :, 0:half, :])
            new_half = x0[:, :, half:, :]
            gen.append(new_half)
        return torch.stack(gen, dim=1)

    @torch.no_grad()
    def predict_joint(self, cond: torch.Tensor, cond_mid: Optional[torch.Tensor] = None, uncond_scale=1.0, orig=None, mask=None,
                      cond_concat=None, noise: Optional[torch.Tensor] = None, blend: str = "mean"):
        """All ``2B-1`` half-overlapping 8-bar windows of every song in ONE reverse loop on one canvas per song (``sampler.WindowPlan``;
        MultiDiffusion along the time axis; not in the reference), where ``predict_songs`` makes ``2B-1`` sampling runs one after the other.

        Inputs as ``predict_songs``: ``cond`` / ``cond_mid`` ``[S, B, n_cond, d_cond]`` as ``encode_conditions(..., autoreg=True)`` returns
        them per song - window ``w`` of song ``s`` takes ``cond[s, w / 2]`` for even ``w`` (the aligned segments) and ``cond_mid[s, (w - 1) / 2]``
        for odd ``w`` (the half-shifted ones; the wrapped last row of ``cond_mid`` is unused, as under ``--autoreg``); ``orig`` / ``mask`` /
        ``noise`` / ``cond_concat``, when given, ``[S, B, C, H, W]``, stitched along the time axis into canvases of ``H * B`` rows.  The
        sampler's draws are keyed by (seed, draw counter, global song index), so ranks that shard the songs reproduce the unsharded run.
        A song of one segment is one window: the bits of ``predict``.  Returns ``[S, B, C, H, W]``."""
        from .sampler import WindowPlan
        p, dev = self.params, cond.device
        S, B = cond.shape[0], cond.shape[1]
        H = p.img_h
        plan = WindowPlan(2 * B - 1, H // 2, H, blend)
        if B > 1 and (cond_mid is None or cond_mid.shape[:2] != cond.shape[:2]):
            raise ValueError("predict_joint: songs of more than one segment need cond_mid, the conditions of the half-shifted windows, shaped like cond")
        wins = [cond[:, w // 2] if w % 2 == 0 else cond_mid[:, (w - 1) // 2] for w in range(plan.n_windows)]
        cw = torch.stack(wins, dim=1).reshape(S * plan.n_windows, *cond.shape[2:]).contiguous()
        # [S, B, C, H, W] -> the canvas [S, C, B * H, W] and back
        stitch = lambda v: None if v is None else v.permute(0, 2, 1, 3, 4).reshape(S, v.shape[2], B * H, v.shape[4]).contiguous().float()
        shape = [S, p.out_channels, plan.canvas_h, p.img_w]
        if orig is None or mask is None:
            orig, mask = torch.zeros(shape, device=dev), torch.zeros(shape, device=dev)
        else:
            orig, mask = stitch(orig), stitch(mask)
        noise = self.sampler.randn(shape, dev) if noise is None else stitch(noise)
        uc = -torch.ones([S * plan.n_windows, 1, p.d_cond], device=dev)
        before = getattr(self.sampler, "windows", None)
        self.sampler.windows = plan
        try:
            xt = self.sampler.q_sample(orig, self.t_idx, noise)
            x0 = self.sampler.paint(xt, cw, self.t_idx, orig=orig, mask=mask, orig_noise=noise, uncond_scale=uncond_scale, uncond_cond=uc,
                                    cond_concat=stitch(cond_concat), repaint_n=self.repaint_n)
        finally:
            self.sampler.windows = before
        return x0.reshape(S, x0.shape[1], B, H, x0.shape[3]).permute(0, 2, 1, 3, 4).contiguous()

    @torch.no_grad()
    def edit(self, orig: torch.Tensor, cond_src: torch.Tensor, cond_tgt: torch.Tensor, uncond_scale=1.0, *, iters: int = 3,
             depth: Optional[int] = None, invert_scale=None, cond_mid_src: Optional[torch.Tensor] = None,
             cond_mid_tgt: Optional[torch.Tensor] = None, joint: bool = False, blend: str = "mean", roundtrip: bool = False):
        """Edit a given song by exact DDIM inversion (``DDIMSampler.invert``; not in the reference): walk ``orig`` ``[B, C, H, W]`` up the
        eta = 0 ODE under its own condition ``cond_src`` to index ``depth`` (default: the run's start index), then ``paint`` back down under
        ``cond_tgt``.  Where inpainting keeps a masked region and invents the rest, this keeps the whole song recognisable and changes what
        the condition changes.  ``iters``: fixed-point iterates per upward step; ``invert_scale``: the guidance scale of the upward walk
        (default: ``uncond_scale``, which also makes ``cond_tgt == cond_src`` the round trip).  ``joint``: the song as ONE canvas with the
        window plan of ``predict_joint`` (``cond_mid_*``: the conditions of the half-shifted windows).  Returns the edited image
        ``[B, C, H, W]``; with ``roundtrip`` also the repaint under ``cond_src`` at the inversion's scale, which a converged inversion
        brings back to ``orig``.  The residuals of the walk stay in ``self.sampler.last_inversion``."""
        s, p = self.sampler, self.params
        if not isinstance(s, DDIMSampler):
            raise ValueError("edit: exact inversion exists for the DDIM sampler with eta = 0 only")
        depth = self.t_idx if depth is None else int(depth)
        inv_scale = uncond_scale if invert_scale is None else invert_scale
        orig = orig.contiguous().float()
        B, H, dev = orig.shape[0], p.img_h, orig.device
        if not joint:
            uc = -torch.ones([B, 1, p.d_cond], device=dev)
            x = s.invert(orig, cond_src, depth, iters=iters, uncond_scale=inv_scale, uncond_cond=uc)
            out = s.paint(x, cond_tgt, depth, uncond_scale=uncond_scale, uncond_cond=uc)
            return (out, s.paint(x, cond_src, depth, uncond_scale=inv_scale, uncond_cond=uc)) if roundtrip else out
        from .sampler import WindowPlan
        plan = WindowPlan(2 * B - 1, H // 2, H, blend)
        if B > 1 and (cond_mid_src is None or cond_mid_tgt is None):
            raise ValueError("edit: a joint edit of more than one segment needs cond_mid_src and cond_mid_tgt, the conditions of the half-shifted windows")
        windows = lambda c, m: torch.stack([c[w // 2] if w % 2 == 0 else m[(w - 1) // 2] for w in range(plan.n_windows)]).contiguous()
        canvas = orig.permute(1, 0, 2, 3).reshape(1, orig.shape[1], B * H, orig.shape[3]).contiguous()
        uc = -torch.ones([plan.n_windows, 1, p.d_cond], device=dev)
        back = lambda v: v.reshape(v.shape[1], B, H, v.shape[3]).permute(1, 0, 2, 3).contiguous()
        before = getattr(s, "windows", None)
        s.windows = plan
        try:
            cs, ct = windows(cond_src, cond_mid_src), windows(cond_tgt, cond_mid_tgt)
            x = s.invert(canvas, cs, depth, iters=iters, uncond_scale=inv_scale, uncond_cond=uc)
            out = back(s.paint(x, ct, depth, uncond_scale=uncond_scale, uncond_cond=uc))
            return (out, back(s.paint(x, cs, depth, uncond_scale=inv_scale, uncond_cond=uc))) if roundtrip else out
        finally:
            s.windows = before

    @torch.no_grad()
    def morph(self, orig_a: Optional[torch.Tensor], cond_a: torch.Tensor, orig_b: Optional[torch.Tensor], cond_b: torch.Tensor,
              frames: int = 5, uncond_scale=1.0, *, iters: int = 3, depth: Optional[int] = None, ease: str = "linear", cond_how: str = "lerp",
              joint: bool = False, blend: str = "mean", cond_mid_a: Optional[torch.Tensor] = None, cond_mid_b: Optional[torch.Tensor] = None):
        """``frames`` songs on a path from song A to song B (``DDIMSampler.morph``; not in the reference): ``orig_a`` / ``orig_b`` ``[B, C, H,
        W]`` are walked up the eta = 0 ODE under their own conditions to index ``depth`` (default: the run's start index), the noises
        interpolated on the sphere and the conditions as ``cond_how`` says, every frame painted back down.  Without the two images
        (``None``) the end noises are two fresh draws (``morph_from_noise``: DDIM with eta 0 or DPM-Solver++).  ``joint``: each song as
        ONE canvas with the window plan of ``predict_joint`` (``cond_mid_*``: the conditions of the half-shifted windows).  Returns
        ``[K, B, C, H, W]``; the slerp tables and the inversion's residuals stay in ``self.sampler.last_morph``."""
        s, p = self.sampler, self.params
        if (orig_a is None) != (orig_b is None):
            raise ValueError("morph: both songs' images, or neither (a path between two noise draws)")
        if orig_a is not None and not isinstance(s, DDIMSampler):
            raise ValueError("morph: exact inversion exists for the DDIM sampler with eta = 0 only")
        depth = self.t_idx if depth is None else int(depth)
        B, H, dev = cond_a.shape[0], p.img_h, cond_a.device
        kw = dict(ease=ease, cond_how=cond_how, uncond_scale=uncond_scale)
        if not joint:
            uc = -torch.ones([B, 1, p.d_cond], device=dev)
            if orig_a is None:
                return s.morph_from_noise([B, p.out_channels, H, p.img_w], cond_a, cond_b, frames, t_start=depth, uncond_cond=uc, **kw)
            return s.morph(orig_a.contiguous().float(), cond_a, orig_b.contiguous().float(), cond_b, frames, t_end=depth, iters=iters,
                           uncond_cond=uc, **kw)
        from .sampler import WindowPlan
        plan = WindowPlan(2 * B - 1, H // 2, H, blend)
        if B > 1 and (cond_mid_a is None or cond_mid_b is None):
            raise ValueError("morph: a joint morph of more than one segment needs cond_mid_a and cond_mid_b, the conditions of the half-shifted windows")
        windows = lambda c, m: torch.stack([c[w // 2] if w % 2 == 0 else m[(w - 1) // 2] for w in range(plan.n_windows)]).contiguous()
        canvas = lambda v: v.contiguous().float().permute(1, 0, 2, 3).reshape(1, v.shape[1], B * H, v.shape[3]).contiguous()
        uc = -torch.ones([plan.n_windows, 1, p.d_cond], device=dev)
        before = getattr(s, "windows", None)
        s.windows = plan
        try:
            ca, cb = windows(cond_a, cond_mid_a), windows(cond_b, cond_mid_b)
            if orig_a is None:
                out = s.morph_from_noise([1, p.out_channels, plan.canvas_h, p.img_w], ca, cb, frames, t_start=depth, uncond_cond=uc, **kw)
            else:
                out = s.morph(canvas(orig_a), ca, canvas(orig_b), cb, frames, t_end=depth, iters=iters, uncond_cond=uc, **kw)
        finally:
            s.windows = before
        K = out.shape[0]                                                     # [K, 1, C, B * H, W] -> [K, B, C, H, W]
        return out.reshape(K, out.shape[2], B, H, out.shape[4]).permute(0, 2, 1, 3, 4).contiguous()

    def _stamp(self, uncond_scale, autoreg, extra="", joint=None):
        """``joint``: ``None``, or the blend of a joint run (``mean`` is written as plain ``joint``)."""
        how = ",autoreg" if autoreg else "" if not joint else ",joint" if joint == "mean" else f",joint-{joint}"
        # the sampler's guidance settings, only when set: without them the name is what it always was
        phi, interval = getattr(self.sampler, "guidance_rescale", 0.0), getattr(self.sampler, "guidance_interval", None)
        how += (f",rescale={phi}" if phi else "") + (f",interval={interval[0]}-{interval[1]}" if interval is not None else "")
        th = getattr(self.sampler, "x0_threshold", None)
        how += "" if th is None else f",{th.label}"
        eta = getattr(self.sampler, "eta", 0.0) if isinstance(self.sampler, DPMSolverSampler) else 0.0
        how += f",dpm_eta={eta:g}" if eta else ""
        st = getattr(self.sampler, "steering", None)
        how += "" if st is None else f",{st.label}"
        return (f"{self.model_label}{extra}[scale={uncond_scale}{how}]"
                f"_{datetime.now().strftime('%y-%m-%d_%H%M%S')}")

    def generate(self, cond, cond_mid=None, uncond_scale=1.0, autoreg=False, no_output=False, cond_concat=None,
                 output_dir="exp", **_ignored):
        gen = self.predict(cond, cond_mid, uncond_scale, autoreg, cond_concat=cond_concat)
        if not no_output:
            os.makedirs(output_dir, exist_ok=True)
            stamp = os.path.join(output_dir, self._stamp(uncond_scale, autoreg))
            np.save(stamp + ".npy", gen.cpu().numpy())
            midi.prmat2c_to_midi_file(gen, stamp + ".mid")            # ref:inference_sdf.py:335-338
        return gen

    def inpaint(self, orig, inpaint_type, cond, cond_mid=None, autoreg=False, orig_noise=None, uncond_scale=1.0,
                bar_list=None, no_output=False, cond_concat=None, output_dir="exp"):
        mask = get_mask(orig, inpaint_type, bar_list).to(orig.device)
        gen = self.predict(cond, cond_mid, uncond_scale, autoreg, orig, mask, cond_concat=cond_concat, noise=orig_noise)
        if not no_output:
            os.makedirs(output_dir, exist_ok=True)
            stamp = os.path.join(output_dir, self._stamp(uncond_scale, autoreg, f"_inp{self.repaint_n}_{inpaint_type}"))
            np.save(stamp + ".npy", gen.cpu().numpy())
            midi.prmat2c_to_midi_file(gen, stamp + ".mid", inp_mask=mask)   # ref:inference_sdf.py:385-389: generated cells on their own track
        return gen


# --------------------------------------------------------------------------------------------- assembly
def build_unet(params, device=None, x3=None) -> UNetModel:
    """`x3="f16"`: the model lives in the fp16-split build of the library (its split mode is "f16x3", UNetModel.__init__)."""
    return UNetModel(in_channels=params.in_channels, out_channels=params.out_channels, channels=params.channels,
                     attention_levels=params.attention_levels, n_res_blocks=params.n_res_blocks,
                     channel_multipliers=params.channel_multipliers, n_heads=params.n_heads, tf_layers=params.tf_layers,
                     d_cond=params.d_cond, img_h=params.img_h, img_w=params.img_w, device=device, x3=x3)


PRECISION_PROBE_TOL = 3e-4
F16_HEADROOM_MIN = 8.0       # f16x3 is kept only if 65504 / max|stored activation| on the probe is at least this


def pick_precision(unet: UNetModel, cond: torch.Tensor, tol: Optional[float] = None, n_steps: int = 1000, seed: int = 0):
    """``--precision auto``: choose the arithmetic mode by MEASURING this network.  bf16x3 (three bf16 MFMAs per product, unit
    roundoff ~2^-18) is ~3x faster than the exact-fp32-MFMA mode and sits 5e-5 from the reference on ordinarily-conditioned
    weights, but every rounding error is amplified by the network's conditioning - fp32's too - and on badly-scaled weights the
    split can exceed the 1e-3 contract (tests/test_gpu_long_parity.py, tools/stress_diag.py).  One evaluation in each mode on three
    probe samples (Gaussian x at t = n_steps-1, n_steps/2 and 0, the first rows of the run's own ``cond``); bf16x3 is kept only if
    ``max|eps_bf16x3 - eps_f32| <= tol * max|eps_f32|`` (default 3e-4: a third of the contract).  Sets the mode on ``unet`` and
    returns ``(mode, measured ratio)``.  Cost: two evaluations of a loop that runs 50-1000."""
    lib = _lib.load()
    tol = PRECISION_PROBE_TOL if tol is None else tol
    n = 3
    x = torch.empty(n, unet.cfg.in_channels, unet.img_h, unet.img_w, dtype=torch.float32, device=cond.device)
    _lib.check(lib.pf_randn(x.data_ptr(), x.numel(), int(seed) + 0x5eed, 0, 0, _lib.current_stream()), "pf_randn")
    t = torch.tensor([n_steps - 1, n_steps // 2, 0], device=cond.device)
    c = cond[torch.arange(n, device=cond.device) % cond.shape[0]].contiguous()
    unet.set_precision("f32")
    # the f32 evaluation doubles as the range measurement: the largest |value| any layer stores (pf_unet_track_absmax).  In the fp16-piece
    # build such a value overflows beyond 65504; measured in f32 nothing overflows while measuring.  A model of the fp16 build must show
    # F16_HEADROOM_MIN x headroom on the probe to be kept in f16x3 - the probe inputs are three samples, a loop sees a thousand.
    unet.track_absmax(True)
    ref = unet(x, t, c).clone()
    absmax = unet.read_absmax()
    unet.track_absmax(False)
    pick_precision.last_absmax = absmax
    unet.set_precision(unet.split_mode)     # "bf16x3", or "f16x3" for a model built in the fp16-split library
    got = unet(x, t, c)
    scale = ref.abs().max().item()
    ratio = float("inf") if not (scale > 0 and bool(torch.isfinite(got).all())) else (got - ref).abs().max().item() / scale
    if unet.split_mode == "f16x3" and not (absmax * F16_HEADROOM_MIN <= 65504.0):
        ratio = float("inf")                # too close to fp16's range (or already beyond it: nan / inf compare false)
    mode = unet.split_mode if ratio <= tol else "f32"
    unet.set_precision(mode)
    return mode, ratio


pick_precision.last_absmax = float("nan")


def build_ldm(params, unet: UNetModel) -> LatentDiffusion:
    return LatentDiffusion(linear_start=params.linear_start, linear_end=params.linear_end, n_steps=params.n_steps,
                           latent_scaling_factor=params.latent_scaling_factor, autoencoder=None, unet_model=unet)


def build_encoders(params, device=None):
    chord_enc = txt_enc = None
    if "chord" in params.cond_type and params.use_enc:
        chord_enc = ChordEncoder(params.chd_input_dim, params.chd_hidden_dim, params.chd_z_dim, device)
    if "txt" in params.cond_type and params.use_enc:
        txt_enc = TextureEncoder(params.txt_emb_size, params.txt_hidden_dim, params.txt_z_dim, params.txt_num_channel, device)
    return chord_enc, txt_enc


def build_pnotree_encoder(params, device=None):
    """The frozen PianoTree encoder of the sdf_pnotree variant (ref:inference_sdf.py:676-680; default sizes, max_simu_note 20)."""
    from .model_sdf import PianoTreeEncoder
    return PianoTreeEncoder(max_simu_note=20, device=device) if params.cond_type == "pnotree" else None


def synthetic_model(params, seed: int = 0, device=None, x3=None) -> Polyffusion_SDF:
    """Whole model with deterministic synthetic weights (same generator as the golden vectors)."""
    from .arch import UNetConfig
    from .weights import synth_chord_encoder_state, synth_texture_encoder_state, synth_unet_state
    unet = build_unet(params, device, x3)
    unet.load_state_dict(synth_unet_state(UNetConfig.from_params(params), seed))
    chord_enc, txt_enc = build_encoders(params, device)
    if chord_enc is not None:
        chord_enc.load_state_dict(synth_chord_encoder_state(seed, params.chd_input_dim, params.chd_hidden_dim, params.chd_z_dim))
    if txt_enc is not None:
        txt_enc.load_state_dict(synth_texture_encoder_state(seed, params.txt_emb_size, params.txt_hidden_dim,
                                                            params.txt_z_dim, params.txt_num_channel))
    pnotree_enc = build_pnotree_encoder(params, device)
    if pnotree_enc is not None:
        from .weights import synth_pianotree_encoder_state
        pnotree_enc.load_state_dict(synth_pianotree_encoder_state(seed))
    return Polyffusion_SDF(build_ldm(params, unet), params.cond_type, params.cond_mode, chord_enc=chord_enc, txt_enc=txt_enc,
                           pnotree_enc=pnotree_enc)


def encode_conditions(model: Polyffusion_SDF, params, chd, prmat, autoreg: bool, pnotree=None):
    cond_mid = None
    if params.cond_type == "pnotree":          # ref:inference_sdf.py:756-760
        assert pnotree is not None
        cond = model._encode_pnotree(pnotree)
        if autoreg:
            cond_mid = model._encode_pnotree(get_autoreg_data(pnotree))
    elif params.cond_type == "chord":
        assert chd is not None
        cond = model._encode_chord(chd)
        if autoreg:
            cond_mid = model._encode_chord(get_autoreg_data(chd))
    elif params.cond_type == "txt":
        assert prmat is not None
        cond = model._encode_txt(prmat)
        if autoreg:
            cond_mid = model._encode_txt(get_autoreg_data(prmat))
    elif params.cond_type == "chord+txt":
        assert chd is not None and prmat is not None
        n = min(chd.shape[0], prmat.shape[0])
        chd, prmat = chd[:n], prmat[:n]
        zchd = model._encode_chord(chd)
        model.cond_split = int(zchd.shape[-1])       # where the texture part begins (DualScale.split: read here, where the two are joined)
        cond = torch.cat([zchd, model._encode_txt(prmat)], dim=-1)
        if autoreg:
            cond_mid = torch.cat([model._encode_chord(get_autoreg_data(chd)), model._encode_txt(get_autoreg_data(prmat))], dim=-1)
    else:
        raise NotImplementedError(f"cond_type {params.cond_type!r} is outside the rebuilt path")
    return cond, cond_mid


def make_parser() -> ArgumentParser:
    p = ArgumentParser(description="inference a Polyffusion model (MI355X-native denoising path)")
    p.add_argument("--chkpt_path", help="the path of the checkpoint to be used")
    p.add_argument("--custom_params_path", help="params yaml/json; default <chkpt>/../../params.yaml")
    p.add_argument("--uncond_scale", type=float, default=1.0, help="unconditional scale for classifier-free guidance")
    # extension: dual guidance for chord+txt models (sampler.DualScale) - what cond_mode mix2 trains for
    p.add_argument("--uncond_scale_chd", type=float, default=None, metavar="X", help="extension, chord+txt models, together with "
                   "--uncond_scale_txt: separate guidance scales for the chord and the texture part of the condition.  With the default "
                   "--guidance_order chd,txt: eps = eps(-,-) + X * (eps(chd,-) - eps(-,-)) + Y * (eps(chd,txt) - eps(chd,-)); with txt,chd: "
                   "eps = eps(-,-) + Y * (eps(-,txt) - eps(-,-)) + X * (eps(chd,txt) - eps(-,txt)) ('-' = that part dropped, as cond_mode "
                   "mix2 trains it).  X == Y is --uncond_scale X; costs three denoiser evaluations per step instead of two")
    p.add_argument("--uncond_scale_txt", type=float, default=None, metavar="Y", help="extension: the texture scale Y of --uncond_scale_chd")
    p.add_argument("--guidance_rescale", type=float, default=0.0, metavar="PHI", help="extension: guidance rescale (Lin et al. 2024, section "
                   "3.4): the guided prediction is scaled back to the conditional prediction's per-sample standard deviation and mixed with the "
                   "plain one by PHI in [0, 1] (0, the default: off; 0.7 is the paper's).  Per window under --joint.  No effect without guidance")
    p.add_argument("--guidance_interval", type=float, nargs=2, default=None, metavar=("LO", "HI"), help="extension: guide only while the time "
                   "step lies in the fractions [LO, HI] of the schedule, 0 <= LO <= HI <= 1 (Kynkaanniemi et al. 2024): t_lo = ceil(LO * (T - 1)), "
                   "t_hi = floor(HI * (T - 1)); outside it a step evaluates the condition alone, at the plain batch.  Not with --hip_graph")
    p.add_argument("--x0_clip", action="store_true", help="extension: clip the predicted clean image to --x0_range at every step (clip_denoised "
                   "of Ho et al. 2020), as a rewrite of the noise prediction.  Goes wherever --uncond_scale goes")
    p.add_argument("--x0_threshold", type=float, default=None, metavar="P", help="extension: dynamic thresholding (Saharia et al. 2022, section "
                   "2.3): at every step each sample's predicted clean image is clipped at the P-quantile (0 < P <= 1; 0.995 is the paper's) of its "
                   "own distances from the centre of --x0_range, never below the range's half-width, and scaled back into the range.  Per song "
                   "canvas under --joint.  Not together with --x0_clip")
    p.add_argument("--x0_range", type=float, nargs=2, default=None, metavar=("LO", "HI"), help="extension: the data range of --x0_clip / "
                   "--x0_threshold, LO < HI (default: 0 1, the range of prmat2c)")
    p.add_argument("--x0_threshold_max", type=float, default=None, metavar="R", help="extension: cap the threshold of --x0_threshold at R >= 1 "
                   "times the range's half-width (default: no cap)")
    p.add_argument("--guidance_order", choices=list(GUIDANCE_ORDERS), default="chd,txt", metavar="{chd,txt | txt,chd}", help="extension: which part the intermediate "
                   "evaluation of --uncond_scale_chd / --uncond_scale_txt keeps (the part named first); default: chd,txt")
    p.add_argument("--seed", type=int, help="use a specific seed for inference")
    joins = p.add_mutually_exclusive_group()     # two ways to join the segments of a song: argparse refuses the pair
    joins.add_argument("--autoreg", action="store_true", help="autoregressively inpaint the music segments")
    # extension: all 2B-1 half-overlapping windows of a song denoised as one batch in ONE reverse loop (sampler.WindowPlan)
    joins.add_argument("--joint", action="store_true", help="extension: denoise all 2B-1 half-overlapping 8-bar windows of a song jointly in one "
                       "reverse loop, their noise predictions blended where they overlap (one sampling run where --autoreg makes 2B-1; "
                       "not together with --autoreg)")
    p.add_argument("--joint_blend", choices=["mean", "ramp"], default="mean", help="extension: how --joint weights two windows over the same "
                   "rows: mean (default) or ramp (a window fades in and out linearly over its overlaps)")
    p.add_argument("--from_dataset", default=None, help="choose condition from a dataset {pop909, musicalion} (validation half of its split)")
    p.add_argument("--dataset_dir", help="extension: directory of the dataset's song .npz files (default: the reference's dirs.py paths)")
    p.add_argument("--split_dir", default=datasample.TRAIN_SPLIT_DIR, help="extension: directory of the <dataset>.pickle split files")
    p.add_argument("--song_index", type=int, help="extension: index into the validation list (the reference asks on the terminal)")
    p.add_argument("--song_index2", type=int, help="extension: the same for the texture song of chord+txt models")
    p.add_argument("--inpaint_song_index", type=int, help="extension: the same for --inpaint_from_dataset")
    p.add_argument("--from_midi", help="choose condition from a midi file")
    p.add_argument("--from_midi2", help="choose condition from the 2nd midi file. Used for chord+txt conditioning")
    p.add_argument("--inpaint_from_midi", help="inpaint a midi file")
    p.add_argument("--inpaint_from_dataset", default=None, help="inpaint a song from a dataset {pop909, musicalion}")
    p.add_argument("--inpaint_pop909_use_track", help="which tracks to use as base song for inpainting, default: 0,1,2")
    p.add_argument("--inpaint_type", help="inpaint a song, type: {remaining, below, above, bars}")
    p.add_argument("--ddim", action="store_true", help="whether to use DDIM sampler")
    p.add_argument("--ddim_discretize", default="uniform", help="{uniform(default), quad}")
    p.add_argument("--ddim_eta", type=float, default=0.0, help="ddim eta, default: 0.0")
    p.add_argument("--ddim_steps", type=int, default=50, help="number of ddim sampling steps, default: 50")
    # extension: DPM-Solver++(2M), a second-order solver of the ODE that --ddim (eta 0) solves to first order, at the same cost per step
    p.add_argument("--dpm", action="store_true", help="extension: use the DPM-Solver++(2M) sampler (not together with --ddim)")
    p.add_argument("--dpm_steps", type=int, default=20, help="number of DPM-Solver++ sampling steps, default: 20 (the logsnr grid drops "
                   "repeated time steps, so it can run fewer)")
    p.add_argument("--dpm_order", type=int, choices=[1, 2], default=2, help="solver order, default: 2 (1 = DDIM with eta 0 on the same grid)")
    p.add_argument("--dpm_discretize", choices=["logsnr", "uniform", "quad"], default="logsnr", help="time-step grid: uniform in log-SNR "
                   "(default; what the second-order update needs to pay off) or DDIM's two grids")
    p.add_argument("--dpm_eta", type=float, default=0.0, metavar="ETA", help="with --dpm: the stochastic form of the solver - 0 (default) is the "
                   "deterministic sampler, 1 is SDE-DPM-Solver++(2M) (\"DPM++ 2M SDE\"), in between interpolates; every step then draws noise, "
                   "so --steer works with it and --morph does not")
    # extension: edit the condition song itself by exact DDIM inversion (DDIMSampler.invert) - e.g. re-harmonise it
    p.add_argument("--edit", action="store_true", help="extension: edit the condition song's own image (from --from_midi, --from_dataset, "
                   "--from_song_npz or prmat2c in --cond_npz) instead of generating from noise: invert it up the eta = 0 DDIM ODE under its own "
                   "condition, sample back down with its chords replaced (--edit_chord_shift / --edit_chords_from_midi).  Needs --ddim with "
                   "--ddim_eta 0 and a chord or chord+txt model")
    p.add_argument("--edit_iters", type=int, default=3, metavar="K", help="fixed-point iterates (denoiser evaluations) per upward step, "
                   "default: 3 (1 = the naive explicit inversion, which falls apart under guidance above 1)")
    p.add_argument("--edit_depth", type=int, default=None, metavar="D", help="grid index to invert to, default: the full range "
                   "(--ddim_steps - 1); lower keeps more of the song")
    p.add_argument("--edit_invert_scale", type=float, default=None, metavar="S", help="guidance scale of the upward walk, default: the run's scale")
    p.add_argument("--edit_roundtrip", action="store_true", help="also sample back under the song's own condition and print max |x - x_rec| "
                   "and the number of note cells > 0.5 that differ")
    p.add_argument("--edit_chord_shift", type=int, default=None, metavar="N", help="target chords: the song's own with each of the three "
                   "12-wide blocks (root, chroma, bass) rolled by N semitones")
    p.add_argument("--edit_chords_from_midi", default=None, metavar="FILE", help="target chords: those of another midi file")
    # extension: a path between two songs - invert both, interpolate their noises on the sphere and their conditions, sample every point
    p.add_argument("--morph", action="store_true", help="extension: write --morph_frames songs on a path from the condition song (A) to a "
                   "second one (B: --morph_to_midi, --morph_to_song_index or --morph_to_npz): both are inverted up the eta = 0 DDIM ODE under "
                   "their own conditions, the noises interpolated spherically, the encoded conditions as --morph_cond says, every frame "
                   "sampled back down.  Needs --ddim with --ddim_eta 0.  With --synthetic (no song images) the path runs between two "
                   "fresh noise draws under two synthetic conditions; that also works with --dpm")
    p.add_argument("--morph_frames", type=int, default=5, metavar="K", help="frames of the path, both songs included: 2..64, default 5")
    p.add_argument("--morph_ease", choices=list(MORPH_EASES), default="linear", help="where the frames sit between A and B: evenly (linear, "
                   "default) or slow at both ends (cosine)")
    p.add_argument("--morph_iters", type=int, default=3, metavar="N", help="fixed-point iterates per upward step of the two inversions, default: 3")
    p.add_argument("--morph_depth", type=int, default=None, metavar="D", help="grid index to invert to and sample from, default: the full range")
    p.add_argument("--morph_cond", choices=list(MORPH_CONDS), default="lerp", help="the frames' conditions: the two encoded conditions "
                   "interpolated linearly (lerp, default) or A's up to the middle and B's from there (switch)")
    p.add_argument("--morph_to_midi", default=None, metavar="FILE", help="song B: a midi file")
    p.add_argument("--morph_to_song_index", type=int, default=None, metavar="N", help="song B: index into the validation list of --from_dataset")
    p.add_argument("--morph_to_npz", default=None, metavar="FILE", help="song B: an npz with chord [B,32,36] and prmat2c [B,2,128,128] "
                   "(and prmat [B,128,128] for chord+txt models; default: song A's texture)")
    p.add_argument("--repaint_n", type=int, default=1, help="n sampling steps in RePaint")
    p.add_argument("--length", type=int, default=0, help="the generated length (in 8-bars)")
    p.add_argument("--show_image", action="store_true", help="(ignored: no image writer on this path)")
    p.add_argument("--chkpt_name", default="weights_best.pt")
    p.add_argument("--num_generate", type=int, default=1, help="the number of samples to generate")
    p.add_argument("--output_dir", default="exp", help="directory to store generated piano rolls")
    # extensions of this build
    p.add_argument("--params_preset", help="use a built-in params preset instead of a params.yaml (e.g. sdf_chd8bar)")
    p.add_argument("--synthetic_weights", action="store_true", help="deterministic synthetic weights instead of a checkpoint")
    p.add_argument("--synthetic", action="store_true", help="seeded synthetic chords / textures as conditions")
    p.add_argument("--cond_npz", help="npz with arrays chord [B,32,36] and/or prmat [B,128,128] and/or pnotree [B,128,20,6] (and prmat2c for inpainting)")
    p.add_argument("--from_song_npz", help="a quantised song in the reference's data-dictionary format (notes, start_table, db_pos, "
                   "db_pos_filter, chord - what get_data_for_single_midi / the POP909 .npz files hold): its 8-bar segments supply the "
                   "chord / texture conditions and the image to inpaint (ref:inference_sdf.py:599-610 via data/datasample.py)")
    p.add_argument("--bar_list", help="bars to inpaint for --inpaint_type bars, comma separated")
    p.add_argument("--precision", choices=["auto", "f32", "bf16x3", "f16x3", "auto-f16x3"], default="auto", help="arithmetic of the denoiser's "
                   "contractions: f32 = exact fp32 MFMA; bf16x3 = error-compensated bf16 split (about 3x faster, 5e-5 from the reference on "
                   "ordinarily-conditioned weights); f16x3 = the same split in fp16 pieces (libpfhip_f16.so: fp32-class error at ~0.97 of bf16x3's "
                   "speed, activations must stay below 65504); auto (default) = evaluate f32 and bf16x3 once on this checkpoint and keep bf16x3 "
                   "only if they agree to 3e-4 of the output scale; auto-f16x3 = the same probe for f16x3 (it catches a range overflow)")
    p.add_argument("--no_pnotree_recon", action="store_true", help="cond_type pnotree: do not decode the encoded condition into "
                   "pnotree_recon.mid (the generated songs are the same either way)")
    p.add_argument("--polydis_recon", action="store_true", help="whether to use polydis to reconstruct the generated midi from diffusion model")
    p.add_argument("--polydis", action="store_true", help="use polydis to generate MIDI. For comparison.")
    p.add_argument("--polydis_chd_resample", action="store_true", help="Whether to resample chord with polydis generation")
    p.add_argument("--polydis_path", default=POLYDIS_MODEL_PATH, help="extension: the Polydis checkpoint (the reference hard-codes this path); "
                   "--synthetic_weights selects the synthetic Polydis state instead")
    p.add_argument("--hip_graph", action="store_true", help="capture one reverse step as a hipGraph and replay it (same results; "
                   "removes the host-side launch cost that bounds small batches, e.g. the batch-1 runs of --autoreg)")
    # extension: score the generated rolls against the chords of the run (polyffusion_amd.score; one HIP launch over the images on the device)
    p.add_argument("--score", action="store_true", help="extension: after generation print per song chord_f1, chord_fit, chord_cover, bass_fit, "
                   "integrity and the onset count against the chords the run conditioned on (without chords: the chord-free numbers; when "
                   "inpainting: of the invented cells only) and write <stamp>_score.json.  With --edit: chord_f1 of the source and of the "
                   "edited image, each against the source and against the target chords")
    p.add_argument("--best_of", type=int, default=1, metavar="N", help="extension: generate --num_generate x N candidates (the same songs as "
                   "--num_generate of that product would give), score them and keep the best --num_generate, files named by rank; implies --score")
    p.add_argument("--rank_by", choices=list(pfscore.RANK_BY), default="chord", help="what --best_of ranks by: chord (chord_f1, default), bass "
                   "(bass_fit), integrity (lowest first), texture (rhythm against the texture song; chord+txt models only) or extracted "
                   "(chord_acc of --score_chords: the share of beats whose recognised chord is the conditioning chord) or novelty (copy_score "
                   "of --novelty_corpus, lowest first: the least copied candidates are kept)")
    p.add_argument("--score_bass_relative", action="store_true", help="read the bass block of a chord row as an offset from the root "
                   "(default: an absolute pitch class, as --from_midi writes it)")
    p.add_argument("--score_chords", action="store_true", help="extension, with --score / --best_of: recognise the chords of every generated "
                   "song on the GPU by the rule of --from_midi (polyffusion_amd.chordrec) and compare them with the chords the run conditioned "
                   "on: chord_acc, root_acc, chroma_acc, bass_acc, chroma_iou, the counters and the recognised labels per song, and a "
                   "\"recognized\" key in <stamp>_score.json.  With --edit / --morph: chord_acc beside the chord_f1 numbers")
    # extension: nearest training segment and diversity (polyffusion_amd.rollmatch; pf_roll_pack / pf_roll_match on the images on the device)
    p.add_argument("--novelty_corpus", metavar="FILE", help="extension, with --score / --best_of: a corpus file of python -m "
                   "polyffusion_amd.rollmatch build; every candidate's copy_score (the best Jaccard overlap of its note cells with any corpus "
                   "window under transposition; 1.0: a copy) and its nearest (song, bar, shift) are printed on the song's score line and "
                   "written to <stamp>_score.json.  The mask of an inpainting run is NOT applied: the whole image is compared, so an inpainted "
                   "song's nearest neighbour is expected to be its source.  With --edit / --morph: of the edited image / every frame")
    p.add_argument("--novelty_shifts", type=int, default=6, metavar="S", help="with --novelty_corpus: transpositions of up to S semitones either "
                   "way are tried (0..15, default 6)")
    p.add_argument("--novelty_topk", type=int, default=3, metavar="K", help="with --novelty_corpus: matches kept per image (1..8, default 3; the "
                   "score is the first)")
    p.add_argument("--novelty_plane", choices=list(pfrollmatch.PLANES), default="onset", help="with --novelty_corpus / --diversity: compare "
                   "onset cells (default) or sounding cells (onset | sustain)")
    p.add_argument("--diversity", action="store_true", help="extension, with --score / --best_of: nearest_other per kept song (its best Jaccard "
                   "overlap with any other kept song, no transposition) and the run's diversity = 1 - mean nearest_other")
    # extension: steer the candidates of --best_of while they are sampled (sampler.Steering; pf_x0_predict, pf_steer_resample, pf_rows_gather)
    p.add_argument("--steer", action="store_true", help="extension, with --best_of N > 1: the N consecutive candidates of each kept song are one "
                   "population of a particle filter - every --steer_every steps their predicted clean images are scored and the population is "
                   "resampled in proportion to exp(lambda * reward gain); copies diverge again through their own noise.  The denoiser compute "
                   "is --best_of N's, the final ranking is --best_of's; every song's candidates are sampled as a batch of their own, so the files do not depend "
                   "on the number of GPUs.  Not with --autoreg, --dpm at --dpm_eta 0, --ddim at eta 0 or --hip_graph")
    p.add_argument("--steer_by", choices=list(STEER_BY), default=None, help="the steering reward: chord (chord_f1), bass (bass_fit), integrity "
                   "or texture (default: what --rank_by says, when it is one of these)")
    p.add_argument("--steer_lambda", type=float, default=10.0, metavar="L", help="with --steer: weights are exp(L * reward gain); finite, >= 0 (default 10)")
    p.add_argument("--steer_every", type=int, default=5, metavar="K", help="with --steer: every K-th reverse step is steered (default 5)")
    p.add_argument("--steer_window", type=float, nargs=2, default=None, metavar=("LO", "HI"), help="with --steer: only steps whose time-step value "
                   "lies in this part of the schedule are steered, fractions as --guidance_interval reads them (default: 0 1)")
    p.add_argument("--steer_ess", type=float, default=0.5, metavar="F", help="with --steer: a population is resampled when its effective sample "
                   "size is at most F * N; in (0, 1] (default 0.5)")
    return p


STEER_BY = ("chord", "bass", "integrity", "texture")


def check_steer_args(args, cond_type: Optional[str] = None) -> Optional[dict]:
    """The settings of ``--steer`` as ``Steering`` takes them (``None`` without the flag); every misuse is a ``SystemExit`` with a message,
    raised before any weight is loaded.  ``cond_type``: checked once it is known (``None``: the flags alone)."""
    dflt = make_parser().get_default
    opts = [f"--{k}" for k in ("steer_by", "steer_lambda", "steer_every", "steer_window", "steer_ess") if getattr(args, k, dflt(k)) != dflt(k)]
    if not getattr(args, "steer", False):
        if opts:
            raise SystemExit(f"{', '.join(opts)}: these belong to --steer, which was not given")
        return None
    if getattr(args, "best_of", 1) <= 1:
        raise SystemExit("--steer steers the N candidates of --best_of N: give --best_of N with N > 1")
    if args.best_of > _lib.STEER_MAX_N:
        raise SystemExit(f"--steer with --best_of {args.best_of}: at most {_lib.STEER_MAX_N} candidates per song")
    if getattr(args, "autoreg", False):
        raise SystemExit("--steer with --autoreg: a song is 2B-1 sampling runs one after the other, a population would have to be carried across them (use --joint)")
    if getattr(args, "dpm", False) and float(getattr(args, "dpm_eta", 0.0)) == 0.0:
        raise SystemExit(f"--steer with --dpm: {DPM_STEER_REFUSAL} (give --dpm_eta > 0)")
    if getattr(args, "ddim", False) and float(getattr(args, "ddim_eta", 0.0)) == 0.0:
        raise SystemExit("--steer with --ddim at eta 0: the loop draws no noise, copies of a survivor would never diverge (give --ddim_eta > 0)")
    if getattr(args, "hip_graph", False):
        raise SystemExit("--steer with --hip_graph: a captured step is one launch sequence, the steered and the unsteered step are two")
    if getattr(args, "repaint_n", 1) > 1:
        raise SystemExit("--steer with --repaint_n > 1: a resampled state cannot be re-noised back to the step it came from")
    by = args.steer_by if args.steer_by is not None else args.rank_by
    if by not in STEER_BY:
        raise SystemExit(f"--rank_by {by} is no steering reward (it needs finished songs): give --steer_by, one of {', '.join(STEER_BY)}")
    lam, every, ess = args.steer_lambda, args.steer_every, args.steer_ess
    lo, hi = (0.0, 1.0) if args.steer_window is None else args.steer_window
    if not (math.isfinite(lam) and lam >= 0.0):
        raise SystemExit(f"--steer_lambda {lam}: finite and >= 0")
    if every < 1:
        raise SystemExit(f"--steer_every {every}: at least 1")
    if not 0.0 < ess <= 1.0:
        raise SystemExit(f"--steer_ess {ess}: in (0, 1]")
    if not 0.0 <= lo <= hi <= 1.0:
        raise SystemExit(f"--steer_window {lo} {hi}: fractions of the schedule, 0 <= LO <= HI <= 1")
    if cond_type is not None:
        if by == "texture" and cond_type != "chord+txt":
            raise SystemExit(f"--steer_by texture compares against the texture song of a chord+txt model; this model's cond_type is {cond_type!r}")
        if by in ("chord", "bass") and "chord" not in cond_type.split("+"):
            raise SystemExit(f"--steer_by {by} needs the chords of the run; this model's cond_type is {cond_type!r} (use --steer_by integrity)")
    return dict(reward=by, lam=float(lam), every=int(every), window=(float(lo), float(hi)), ess=float(ess))


def steer_shard(num_generate: int, best_of: int, rank: int, world: int):
    """The candidates ``[lo, hi)`` of rank ``rank`` under ``--steer``: whole groups, ``shard_range(num_generate) * best_of`` - a candidate keeps
    the global index it has in the one-rank run, and so do its group and its noise."""
    from . import dist as pfdist
    lo, hi = pfdist.shard_range(num_generate, rank, world)
    return lo * best_of, hi * best_of


def check_score_args(args, cond_type: Optional[str] = None) -> bool:
    """Whether the command line asks for scores (``--score`` or ``--best_of N > 1``); every misuse is a ``SystemExit`` with a message, raised
    before any weight is loaded.  ``cond_type``: checked once it is known (``None``: the flags alone)."""
    best_of = getattr(args, "best_of", 1)
    if best_of < 1:
        raise SystemExit(f"--best_of {best_of}: at least one candidate per song kept")
    if best_of > 1 and getattr(args, "edit", False):
        raise SystemExit("--best_of with --edit: --edit is deterministic, every candidate would be the same song")
    scoring = bool(getattr(args, "score", False)) or best_of > 1
    dflt = make_parser().get_default
    novelty_opts = [f"--{k}" for k in ("novelty_shifts", "novelty_topk", "novelty_plane") if getattr(args, k, dflt(k)) != dflt(k)]
    if not scoring:
        given = ([f"--{k}" for k in ("score_bass_relative", "score_chords", "novelty_corpus", "diversity") if getattr(args, k, False)] + novelty_opts
                 + (["--rank_by"] if args.rank_by != "chord" else []))
        if given:
            raise SystemExit(f"{', '.join(given)}: these belong to --score / --best_of, which were not given")
        return False
    corpus = getattr(args, "novelty_corpus", None)
    if args.rank_by == "novelty" and best_of > 1 and not corpus:
        raise SystemExit("--rank_by novelty ranks by copy_score, which needs --novelty_corpus FILE")
    if not corpus and [o for o in novelty_opts if o != "--novelty_plane" or not getattr(args, "diversity", False)]:
        raise SystemExit(f"{', '.join(novelty_opts)}: these belong to --novelty_corpus, which was not given")
    if corpus:
        if not 0 <= args.novelty_shifts <= _lib.ROLL_MATCH_MAX_SHIFTS:
            raise SystemExit(f"--novelty_shifts {args.novelty_shifts}: 0..{_lib.ROLL_MATCH_MAX_SHIFTS}")
        if not 1 <= args.novelty_topk <= _lib.ROLL_MATCH_MAX_TOPK:
            raise SystemExit(f"--novelty_topk {args.novelty_topk}: 1..{_lib.ROLL_MATCH_MAX_TOPK}")
    if cond_type is not None:
        if args.rank_by == "texture" and cond_type != "chord+txt":
            raise SystemExit(f"--rank_by texture compares against the texture song of a chord+txt model; this model's cond_type is {cond_type!r}")
        if best_of > 1 and args.rank_by in ("chord", "bass", "extracted") and "chord" not in cond_type.split("+"):
            raise SystemExit(f"--rank_by {args.rank_by} needs the chords of the run; this model's cond_type is {cond_type!r} (use --rank_by integrity)")
    return True


def check_guidance_args(args, n_steps: Optional[int] = None):
    """``(phi, interval)`` of ``--guidance_rescale`` / ``--guidance_interval`` as the samplers take them; every misuse is an argparse error
    (usage + exit status 2).  ``n_steps``: the schedule's length once it is known (``None``: the flags alone, the interval is ``None``)."""
    error = make_parser().error
    phi, fr = getattr(args, "guidance_rescale", 0.0), getattr(args, "guidance_interval", None)
    if not 0.0 <= phi <= 1.0:        # (a NaN fails both)
        error(f"--guidance_rescale {phi}: PHI lies in [0, 1]")
    if fr is None:
        return phi, None
    lo, hi = fr
    if not 0.0 <= lo <= hi <= 1.0:
        error(f"--guidance_interval {lo} {hi}: fractions of the schedule, 0 <= LO <= HI <= 1")
    if getattr(args, "hip_graph", False):
        error("--guidance_interval with --hip_graph: a captured step is one launch sequence, the guided and the unguided step are two")
    if n_steps is None:
        return phi, None
    try:
        return phi, guidance_interval_from_fractions(lo, hi, n_steps)
    except ValueError as e:
        error(f"--guidance_interval {lo} {hi}: {e}")


def check_threshold_args(args) -> Optional[X0Threshold]:
    """The ``X0Threshold`` of ``--x0_clip`` / ``--x0_threshold`` / ``--x0_range`` / ``--x0_threshold_max`` (``None`` without the first two);
    every misuse is an argparse error (usage + exit status 2)."""
    error = make_parser().error
    clip, p = getattr(args, "x0_clip", False), getattr(args, "x0_threshold", None)
    rng, cap = getattr(args, "x0_range", None), getattr(args, "x0_threshold_max", None)
    if clip and p is not None:
        error("--x0_clip and --x0_threshold name two different ways to bound the predicted image: give one of them")
    if not clip and p is None:
        if rng is not None or cap is not None:
            error("--x0_range / --x0_threshold_max without --x0_clip or --x0_threshold: nothing to apply them to")
        return None
    if cap is not None and p is None:
        error("--x0_threshold_max without --x0_threshold: static clipping has no threshold to cap")
    if p is not None and not 0.0 < p <= 1.0:         # (a NaN fails both)
        error(f"--x0_threshold {p}: P lies in (0, 1]")
    if cap is not None and not cap >= 1.0:
        error(f"--x0_threshold_max {cap}: R is at least 1")
    lo, hi = (0.0, 1.0) if rng is None else rng
    if not (math.isfinite(lo) and math.isfinite(hi) and lo < hi):
        error(f"--x0_range {lo} {hi}: LO < HI, both finite")
    return X0Threshold(mode="clip" if clip else "dynamic", p=0.995 if p is None else p, range=(lo, hi), s_max=float("inf") if cap is None else cap)


def wants_dual_guidance(args, cond_type: str) -> bool:
    """Whether the command line asks for dual guidance (``--uncond_scale_chd X --uncond_scale_txt Y``); every misuse is a ``SystemExit``."""
    x, y = getattr(args, "uncond_scale_chd", None), getattr(args, "uncond_scale_txt", None)
    if x is None and y is None:
        return False
    if x is None or y is None:
        raise SystemExit("--uncond_scale_chd and --uncond_scale_txt go together: give both (equal values are --uncond_scale)")
    if cond_type != "chord+txt":
        raise SystemExit(f"--uncond_scale_chd / --uncond_scale_txt steer the two parts of a chord+txt condition; this model's cond_type is "
                         f"{cond_type!r} (use --uncond_scale)")
    if args.uncond_scale != make_parser().get_default("uncond_scale"):
        raise SystemExit("--uncond_scale together with --uncond_scale_chd / --uncond_scale_txt: give the single scale or the two, not both")
    return True


def dual_scale(args, split: int) -> DualScale:
    """The command line's ``DualScale``: X scales the term that brings the chord in and Y the texture's, whichever comes first."""
    x, y = args.uncond_scale_chd, args.uncond_scale_txt
    first, second = (x, y) if args.guidance_order == "chd,txt" else (y, x)
    return DualScale(first, second, split, args.guidance_order)


EDIT_COND_TYPES = ("chord", "chord+txt")


def check_edit_args(args, cond_type: Optional[str] = None, world: int = 1) -> bool:
    """Whether the command line asks for ``--edit``; every misuse is a ``SystemExit`` with a message, raised before any weight is loaded.
    ``cond_type`` / ``world``: checked once they are known (``None`` / 1: the flags alone)."""
    if not getattr(args, "edit", False):
        given = [f"--{k}" for k in ("edit_roundtrip", "edit_chord_shift", "edit_chords_from_midi", "edit_depth", "edit_invert_scale")
                 if getattr(args, k, None) not in (None, False)]
        if given:
            raise SystemExit(f"{', '.join(given)}: these belong to --edit, which was not given")
        return False
    if cond_type is not None and cond_type not in EDIT_COND_TYPES:
        raise SystemExit(f"--edit replaces the chords of a song: it needs a model of cond_type chord or chord+txt, this one's is {cond_type!r}")
    if getattr(args, "dpm", False):
        raise SystemExit("--edit with --dpm: the 2M step's history makes its exact inverse a different problem; use --ddim")
    if not args.ddim:
        raise SystemExit("--edit needs --ddim: only the deterministic DDIM loop (eta 0) has an inverse to walk")
    if args.ddim_eta != 0.0:
        raise SystemExit(f"--edit needs --ddim_eta 0 (got {args.ddim_eta}): a loop that draws noise has no inverse")
    if args.autoreg:
        raise SystemExit("--edit with --autoreg: the autoregressive schedule inpaints from noise; use --joint to edit a song as one canvas")
    if args.inpaint_type is not None:
        raise SystemExit("--edit with --inpaint_type: two different ways to change a song, choose one")
    if args.from_midi2 is not None:
        raise SystemExit("--edit with --from_midi2: the song edited must be described by its own condition (chords and texture of one file)")
    if args.num_generate > 1:
        raise SystemExit("--edit is deterministic: --num_generate > 1 would write the same song again")
    if world > 1:
        raise SystemExit("--edit runs on one rank (one song, one loop)")
    if args.edit_chord_shift is None and args.edit_chords_from_midi is None:
        raise SystemExit("--edit needs the target chords: --edit_chord_shift N or --edit_chords_from_midi FILE")
    if args.edit_chord_shift is not None and args.edit_chords_from_midi is not None:
        raise SystemExit("--edit_chord_shift and --edit_chords_from_midi both name the target chords: give one of them")
    if args.edit_iters < 1:
        raise SystemExit(f"--edit_iters {args.edit_iters}: at least one iterate per step")
    if args.edit_depth is not None and not 0 <= args.edit_depth < args.ddim_steps:
        raise SystemExit(f"--edit_depth {args.edit_depth} outside [0, --ddim_steps - 1 = {args.ddim_steps - 1}]")
    has_image = (args.uncond_scale != 0.0 and (args.from_midi is not None or args.from_dataset is not None)) or args.from_song_npz is not None
    if not has_image and args.cond_npz is not None:        # (main reads --cond_npz only when none of the song sources above is taken)
        with np.load(args.cond_npz) as z:
            has_image = "prmat2c" in z
    if not has_image:
        raise SystemExit("--edit needs the song to edit: --from_midi, --from_dataset, --from_song_npz, or prmat2c in --cond_npz")
    return True


MORPH_TO = ("morph_to_midi", "morph_to_song_index", "morph_to_npz")


def check_morph_args(args, cond_type: Optional[str] = None, world: int = 1) -> bool:
    """Whether the command line asks for ``--morph``; every misuse is a ``SystemExit`` with a message, raised before any weight is loaded.
    ``cond_type`` / ``world``: checked once they are known (``None`` / 1: the flags alone)."""
    dflt = make_parser().get_default
    if not getattr(args, "morph", False):
        given = [f"--{k}" for k in ("morph_frames", "morph_ease", "morph_iters", "morph_depth", "morph_cond") + MORPH_TO
                 if getattr(args, k, dflt(k)) != dflt(k)]
        if given:
            raise SystemExit(f"{', '.join(given)}: these belong to --morph, which was not given")
        return False
    dpm = getattr(args, "dpm", False)
    if not args.ddim and not dpm:
        raise SystemExit("--morph needs --ddim (eta 0) or, between two synthetic conditions, --dpm: the frames of a loop that draws noise are not a path")
    if args.ddim and args.ddim_eta != 0.0:
        raise SystemExit(f"--morph needs --ddim_eta 0 (got {args.ddim_eta}): the frames of a loop that draws noise are not a path")
    if dpm and float(getattr(args, "dpm_eta", 0.0)) != 0.0:
        raise SystemExit(f"--morph needs --dpm_eta 0 (got {args.dpm_eta}): the frames of a loop that draws noise are not a path")
    if args.autoreg:
        raise SystemExit("--morph with --autoreg: the autoregressive schedule inpaints from noise; use --joint to morph songs as canvases")
    if args.inpaint_type is not None:
        raise SystemExit("--morph with --inpaint_type: a morph has no known region, choose one")
    if getattr(args, "edit", False):
        raise SystemExit("--morph with --edit: two different things to do with a song's inversion, choose one")
    if getattr(args, "best_of", 1) > 1:
        raise SystemExit("--best_of with --morph: --morph is deterministic, every candidate would be the same path")
    if args.num_generate > 1:
        raise SystemExit("--morph is deterministic: --num_generate > 1 would write the same path again")
    if world > 1:
        raise SystemExit("--morph runs on one rank (one path, one batch of frames)")
    if not 2 <= args.morph_frames <= _lib.SLERP_MAX_FRAMES:
        raise SystemExit(f"--morph_frames {args.morph_frames} outside [2, {_lib.SLERP_MAX_FRAMES}]")
    if args.morph_iters < 1:
        raise SystemExit(f"--morph_iters {args.morph_iters}: at least one iterate per step")
    steps = args.dpm_steps if dpm else args.ddim_steps
    if args.morph_depth is not None and not 0 <= args.morph_depth < steps:
        raise SystemExit(f"--morph_depth {args.morph_depth} outside [0, {steps - 1}], the sampler's steps")
    to = [f"--{k}" for k in MORPH_TO if getattr(args, k) is not None]
    has_image = (args.uncond_scale != 0.0 and (args.from_midi is not None or args.from_dataset is not None)) or args.from_song_npz is not None
    from_npz = not has_image and args.cond_npz is not None     # (main reads --cond_npz only when none of the song sources above is taken)
    if from_npz:
        with np.load(args.cond_npz) as z:
            has_image = "prmat2c" in z
    if not has_image and not from_npz:
        # no song at all: the path runs between two fresh noise draws under two synthetic conditions
        if not args.synthetic:
            raise SystemExit("--morph needs song A: --from_midi, --from_dataset, --from_song_npz or --cond_npz (or --synthetic for a path "
                             "between two synthetic conditions)")
        if to:
            raise SystemExit(f"{', '.join(to)} with --synthetic: --synthetic morphs between two synthetic conditions, song B is a second draw")
        return True
    if len(to) != 1:
        raise SystemExit(f"--morph needs song B from exactly one of --morph_to_midi, --morph_to_song_index, --morph_to_npz (got {len(to)})")
    if args.morph_to_song_index is not None and args.from_dataset is None:
        raise SystemExit("--morph_to_song_index names a song of --from_dataset, which was not given")
    if not has_image:
        raise SystemExit("--morph needs song A's image: prmat2c in --cond_npz (or --from_midi, --from_dataset, --from_song_npz)")
    if dpm:
        raise SystemExit("--morph with --dpm and a song image: the 2M step has no inverse to walk; use --ddim (or --synthetic, which starts from noise)")
    if cond_type is not None and cond_type not in EDIT_COND_TYPES:
        raise SystemExit(f"--morph between two songs describes each by its chords: it needs a model of cond_type chord or chord+txt, this "
                         f"one's is {cond_type!r}")
    return True


def shift_chords(chd: torch.Tensor, n: int) -> torch.Tensor:
    """``chd [..., 36]`` with each of its three 12-wide blocks (root, chroma, bass) rolled by ``n``: the chords transposed by n semitones."""
    return torch.cat([chd[..., 12 * j: 12 * j + 12].roll(int(n), dims=-1) for j in range(3)], dim=-1)


def polydis_aftertouch(args, say=print):
    """``PolydisAftertouch()`` of ref:inference_sdf.py:340,661 - from ``--polydis_path``, or the synthetic state with
    ``--synthetic_weights``.  Built for one call and dropped by the caller: its blobs and workspaces do not stay on the GPU."""
    from .polydis import PolydisAftertouch
    if args.synthetic_weights:
        from .weights import synth_polydis_state
        return PolydisAftertouch(state=synth_polydis_state(0), say=say)
    return PolydisAftertouch(model_path=args.polydis_path, say=say)


def write_polydis(args, chd, prmat, seed: int, say=print):
    """ref:inference_sdf.py:653-671 (``--polydis``) - the condition song's own texture and chords through Polydis, for comparison:
    ``polydis_prmat.mid`` (the texture as given) and ``polydis_gen.mid`` (its reconstruction) in the output directory (the reference
    writes into ``exp/`` whatever ``--output_dir`` says).  The chord resampling draws from a generator of its own, keyed by the seed."""
    if chd is None or prmat is None:
        raise SystemExit("--polydis needs both the chords and the texture of a condition song (chd and prmat)")
    n = min(chd.shape[0], prmat.shape[0])
    polydis_prmat, polydis_chd = prmat[:n].reshape(-1, 32, 128), chd[:n].reshape(-1, 8, 36)    # 2-bar rows
    os.makedirs(args.output_dir, exist_ok=True)
    p_in, p_gen = os.path.join(args.output_dir, "polydis_prmat.mid"), os.path.join(args.output_dir, "polydis_gen.mid")
    midi.prmat_to_midi_file(polydis_prmat, p_in)
    aftertouch = polydis_aftertouch(args, say)
    aftertouch.reconstruct(polydis_prmat, polydis_chd, p_gen, chd_sample=args.polydis_chd_resample,
                           generator=torch.Generator().manual_seed(seed))
    del aftertouch
    say(f"polydis: {tuple(polydis_prmat.shape)} -> {p_in}, {p_gen}")
    return p_in, p_gen


def write_polydis_recon(args, gen_songs, stamps, chd, say=print):
    """ref:inference_sdf.py:339-348 (``--polydis_recon``) - every generated song's texture with the condition chords through Polydis,
    as ``<stamp>_recon.mid``.  The reference also overwrites ``<stamp>.mid`` with a ``prmat_to_midi_file`` rendering; here the song
    files stay what they are without the flag.  Deterministic (means only): no random numbers."""
    aftertouch = polydis_aftertouch(args, say)
    paths = []
    for song, stamp in zip(gen_songs, stamps):
        prmat = torch.from_numpy(midi.prmat2c_to_prmat(song))                    # [rows, 32, 128]
        polydis_chd = chd.reshape(-1, 8, 36)
        n = min(prmat.shape[0], polydis_chd.shape[0])
        paths.append(stamp + "_recon.mid")
        aftertouch.reconstruct(prmat[:n], polydis_chd[:n], paths[-1])
        say(f"polydis reconstruction: {n} two-bar rows -> {paths[-1]}")
    del aftertouch
    return paths


def write_pnotree_recon(model: Polyffusion_SDF, args, cond, say=print):
    """ref:inference_sdf.py:761-762 - decode the encoded condition back to notes and write ``pnotree_recon.mid`` into the output
    directory: what the condition the denoiser sees actually encodes.  Needs PianoTree decoder weights (synthetic, or
    ``pnotree_dec.*`` keys of the checkpoint); without them one line is printed and the run goes on.  Draws no random numbers."""
    from .model_sdf import PianoTreeDecoder
    if args.synthetic_weights:
        from .weights import synth_pianotree_decoder_state
        state = synth_pianotree_decoder_state(0)
    else:
        state = getattr(model, "pnotree_dec_state", None)      # left by load_model (rank 0) from the checkpoint it read
    model.pnotree_dec_state = None                             # the tensors are needed once
    if not state:
        say("pnotree_recon.mid not written: the checkpoint has no pnotree_dec.* weights")
        return None
    # the decoder lives for this call only: its blob and workspace do not stay on the GPU through sampling
    dec = PianoTreeDecoder(max_simu_note=20).load_state_dict(state)
    grid = Polyffusion_SDF(None, "pnotree", pnotree_dec=dec)._decode_pnotree(cond)
    del dec
    os.makedirs(args.output_dir, exist_ok=True)
    path = os.path.join(args.output_dir, "pnotree_recon.mid")
    midi.estx_to_midi_file(grid, path)
    say(f"condition reconstruction: grid {tuple(grid.shape)} -> {path}")
    return path


def _packed_blobs(params, args, parts, chord_enc, txt_enc):
    """Rank 0's half of ``load_model``: checkpoint (or synthetic) state_dicts -> packed host blobs, one per sub-model; the second
    result is the checkpoint's ``pnotree_dec.*`` part (empty without one), which ``write_pnotree_recon`` uses."""
    from .checkpoint import load_checkpoint, split_state_decoders, split_state_full
    states, pnotree_dec_state = {}, {}
    if args.synthetic_weights:
        from .arch import UNetConfig
        from .weights import synth_chord_encoder_state, synth_pianotree_encoder_state, synth_texture_encoder_state, synth_unet_state
        if params.cond_type == "pnotree":
            states["pnotree_enc"] = synth_pianotree_encoder_state(0)
        states["unet"] = synth_unet_state(UNetConfig.from_params(params), 0)
        if chord_enc is not None:
            states["chord_enc"] = synth_chord_encoder_state(0, params.chd_input_dim, params.chd_hidden_dim, params.chd_z_dim)
        if txt_enc is not None:
            states["txt_enc"] = synth_texture_encoder_state(0, params.txt_emb_size, params.txt_hidden_dim, params.txt_z_dim,
                                                            params.txt_num_channel)
    else:
        path = args.chkpt_path
        if path and os.path.exists(f"{path}/chkpts/{args.chkpt_name}"):
            path = f"{path}/chkpts/{args.chkpt_name}"
        if not path or not (path.endswith(".pt") or path.endswith(".ckpt")):
            raise SystemExit("--chkpt_path must name a legacy .pt or a Lightning .ckpt checkpoint (or a run directory holding chkpts/)")
        full = load_checkpoint(path)[0]
        states = split_state_full(full)
        pnotree_dec_state = split_state_decoders(full)["pnotree_dec"] if params.cond_type == "pnotree" else {}
    blobs = {}
    for name, mod, _ in parts:
        if not states.get(name):
            raise SystemExit(f"checkpoint has no {name} weights")
        blobs[name] = mod.pack_state_dict(states[name])
    return blobs, pnotree_dec_state


def load_model(params, args, rank: int = 0, world: int = 1) -> Polyffusion_SDF:
    """Assemble the model (``inference_sdf.py:536-557,702-734``).  Rank 0 reads the checkpoint (or generates the synthetic
    weights) and repacks it into the kernel-side blobs; with world > 1 the other ranks receive the packed blobs by ONE
    broadcast each (RCCL over xGMI) and never touch the file system - SURVEY.md 8e."""
    from . import _lib, dist as pfdist
    unet = build_unet(params, x3="f16" if getattr(args, "precision", None) in ("f16x3", "auto-f16x3") else None)
    chord_enc, txt_enc = build_encoders(params)
    parts = [("unet", unet, unet.weight_bytes())]
    if chord_enc is not None:
        parts.append(("chord_enc", chord_enc, int(_lib.load().pf_encoder_weight_bytes(chord_enc._h))))
    if txt_enc is not None:
        parts.append(("txt_enc", txt_enc, int(_lib.load().pf_encoder_weight_bytes(txt_enc._h))))
    pnotree_enc = build_pnotree_encoder(params)
    if pnotree_enc is not None:
        parts.append(("pnotree_enc", pnotree_enc, int(_lib.load().pf_encoder_weight_bytes(pnotree_enc._h))))
    dev = _dev()
    blobs, failure, pnotree_dec_state = {}, None, None
    if rank == 0:
        # every failure of the load (bad path, missing sub-model, unexpected / mis-shaped key) happens on rank 0 only while the
        # other ranks already wait for the blobs: catch it, tell them, and let every rank leave with the same message
        try:
            host_blobs, pnotree_dec_state = _packed_blobs(params, args, parts, chord_enc, txt_enc)
            blobs = {name: blob.to(dev) for name, blob in host_blobs.items()}
        except (SystemExit, Exception) as e:   # noqa: BLE001 - re-raised below on every rank
            failure = e
    if pfdist.broadcast_int(0 if failure is None else 1) != 0:
        # ONE exception type on every rank (callers that fall back - `--precision auto` - must take the same branch everywhere)
        if failure is not None:
            if isinstance(failure, SystemExit):
                raise failure
            raise SystemExit(f"could not load the model weights: {type(failure).__name__}: {failure}") from failure
        raise SystemExit("rank 0 could not load the model weights (see its message)")
    for name, mod, nbytes in parts:
        blob = blobs[name] if rank == 0 else torch.empty(nbytes // 4, dtype=torch.float32, device=dev)
        pfdist.broadcast_blob(blob, 0)
        mod.bind_packed(blob)
    model = Polyffusion_SDF(build_ldm(params, unet), params.cond_type, params.cond_mode, chord_enc=chord_enc, txt_enc=txt_enc,
                            pnotree_enc=pnotree_enc)
    model.pnotree_dec_state = pnotree_dec_state or None
    return model


def check_dpm_eta(args) -> float:
    """``--dpm_eta`` as ``DPMSolverSampler`` takes it; a ``SystemExit`` for a value that is not finite and >= 0, or given without ``--dpm``."""
    eta = float(getattr(args, "dpm_eta", 0.0))
    if not (math.isfinite(eta) and eta >= 0.0):
        raise SystemExit(f"--dpm_eta {eta}: finite and >= 0")
    if eta != 0.0 and not getattr(args, "dpm", False):
        raise SystemExit("--dpm_eta belongs to --dpm, which was not given")
    return eta


def make_sampler(model, args, seed: int, sample_offset: int = 0):
    """(sampler, start index) as ``inference_sdf.py:735-747,215-219`` choose them.  Every run's sampler is made here - plain, --autoreg, --joint,
    inpainting, --edit, --morph, --best_of, every rank of a sharded run - so --guidance_rescale / --guidance_interval and
    --x0_clip / --x0_threshold reach all of them."""
    if getattr(args, "dpm", False) and args.ddim:
        raise SystemExit("--dpm and --ddim name two different samplers: give one of them")
    phi, interval = check_guidance_args(args, model.ldm.n_steps)
    guidance = dict(guidance_rescale=phi, guidance_interval=interval, x0_threshold=check_threshold_args(args))
    eta = check_dpm_eta(args)
    if getattr(args, "dpm", False):
        sampler = DPMSolverSampler(model.ldm, args.dpm_steps, args.dpm_discretize, args.dpm_order, seed=seed, sample_offset=sample_offset,
                                   graph=getattr(args, "hip_graph", False), eta=eta, **guidance)
        return sampler, len(sampler.time_steps) - 1      # the grid's own length: logsnr drops repeated time steps
    if args.ddim:
        sampler = DDIMSampler(model.ldm, args.ddim_steps, args.ddim_discretize, args.ddim_eta, seed=seed, sample_offset=sample_offset,
                              graph=getattr(args, "hip_graph", False), **guidance)
        t_idx = args.ddim_steps - 1    # inference_sdf.py:218 (NOT len(time_steps)-1: 'uniform' can yield one more entry)
        if t_idx >= len(sampler.time_steps):
            raise SystemExit(f"--ddim_steps {args.ddim_steps}: the discretisation has only {len(sampler.time_steps)} steps")
        return sampler, t_idx
    return SDFSampler(model.ldm, seed=seed, sample_offset=sample_offset, graph=getattr(args, "hip_graph", False), **guidance), None


def generate_songs(model, params, args, cond, cond_mid, orig, mask, seed: int, rank: int = 0, world: int = 1, cond_concat=None,
                   uncond_scale=None, steer: Optional[dict] = None, chd=None, txt_prmat=None):
    """This rank's share of ``args.num_generate`` (times ``args.best_of``, the candidates of ``--best_of``) independent generations of the
    same conditions.  ``uncond_scale``: the guidance scale
    (``None``: ``args.uncond_scale``; a ``DualScale`` for dual guidance) - handed to the sampler as it is.

    The reference loops over the songs (``inference_sdf.py:774``); here they are ONE batch and the unit of multi-GPU
    sharding: rank r takes the songs ``shard_range(num_generate, r, world)``, keyed into the noise generator by their
    GLOBAL index (``sample_offset``), so the result does not depend on the number of GPUs, and the step loop has no
    collective.  ``steer`` (``check_steer_args``): the ``best_of`` consecutive candidates of a kept song are one steered population
    (``sampler.Steering``) scored against ``chd [B, 32, 36]`` - of the cells ``mask`` marks as invented - or the texture song ``txt_prmat
    [B, H, W]``; the ranks then take whole groups (``steer_shard``) and every group is a ``paint`` call of its own, with a sampler keyed by the
    group's global first sample: what the denoiser computes depends in its last bits on the per-launch batch (it picks its tiles by it), and
    a launch of one group is the same launch whichever rank makes it and however many groups that rank holds - the candidates do not depend
    on the number of GPUs, bit for bit.  The returned Experiments' sampler carries the groups' ``last_steering`` merged.  Returns (``[n_local, B, C, H, W]`` - or ``[n_local, 2B, C, H/2, W]`` with ``--autoreg`` -, the Experiments)."""
    from . import dist as pfdist
    S, B = args.num_generate * getattr(args, "best_of", 1), cond.shape[0]      # --best_of N: N candidates per song kept, all of them songs here
    lo, hi = pfdist.shard_range(S, rank, world) if steer is None else steer_shard(args.num_generate, args.best_of, rank, world)
    joint = getattr(args, "joint", False)
    per_song = 1 if args.autoreg or joint else B   # images (--joint: canvases) the sampler sees per song in one paint() call
    if steer is not None and hi - lo > args.best_of:
        parts = [_generate_block(model, params, args, cond, cond_mid, orig, mask, seed, cond_concat, uncond_scale, g, args.best_of, per_song, joint,
                                 steer, chd, txt_prmat) for g in range(lo, hi, args.best_of)]
        expmt = parts[-1][1]
        expmt.sampler.last_steering = SteeringRecord.merged([e.sampler.last_steering for _, e in parts])
        return torch.cat([g for g, _ in parts]), expmt
    return _generate_block(model, params, args, cond, cond_mid, orig, mask, seed, cond_concat, uncond_scale, lo, hi - lo, per_song, joint, steer, chd, txt_prmat)


def _generate_block(model, params, args, cond, cond_mid, orig, mask, seed, cond_concat, uncond_scale, lo, n_local, per_song, joint, steer, chd, txt_prmat):
    """``generate_songs`` for the ``n_local`` songs from global song ``lo`` on: one sampler, one batch."""
    B = cond.shape[0]
    sampler, t_idx = make_sampler(model, args, seed, lo * per_song)
    if steer is not None and n_local > 0:
        sampler.steering = steering_of(steer, args, n_local, per_song, chd, mask, txt_prmat, joint)
    expmt = Experiments(params.model_name, params, sampler, t_idx=t_idx, repaint_n=args.repaint_n)
    scale = args.uncond_scale if uncond_scale is None else uncond_scale
    rep = lambda v: None if v is None else v.unsqueeze(0).expand(n_local, *v.shape).contiguous()
    C, H, W = params.out_channels, params.img_h, params.img_w
    if n_local == 0:
        gen = torch.empty(0, 2 * B if args.autoreg else B, C, H // 2 if args.autoreg else H, W, device=cond.device)
    elif args.autoreg:
        gen = expmt.predict_songs(rep(cond), rep(cond_mid), scale, orig=rep(orig), mask=rep(mask),
                                  cond_concat=rep(cond_concat))   # [n,2B,C,H/2,W]
    elif joint:
        gen = expmt.predict_joint(rep(cond), rep(cond_mid), scale, orig=rep(orig), mask=rep(mask), cond_concat=rep(cond_concat),
                                  blend=args.joint_blend)         # [n,B,C,H,W]
    else:
        flat = lambda v: None if v is None else rep(v).reshape(n_local * B, *v.shape[1:])
        gen = expmt.predict(flat(cond), None, scale, False, flat(orig), flat(mask),
                            cond_concat=flat(cond_concat)).reshape(n_local, B, C, H, W)
    return gen, expmt


def steering_of(steer: dict, args, n_local: int, per_song: int, chd, mask, txt_prmat, joint: bool) -> Steering:
    """The ``Steering`` of this rank's ``n_local`` candidates: groups of ``args.best_of`` songs of ``per_song`` images (``--joint``: one
    canvas), the reward's chords, mask and texture onsets repeated per candidate in the images' order."""
    rep = lambda v: None if v is None else v.unsqueeze(0).expand(n_local, *v.shape).contiguous()
    if mask is not None and joint:                               # [B, C, H, W] -> the canvas [C, B * H, W], as predict_joint stitches it
        mask = mask.permute(1, 0, 2, 3).reshape(mask.shape[1], -1, mask.shape[3])
    onsets = None
    if steer["reward"] == "texture":
        onsets = (txt_prmat > 0).sum(-1).to(torch.int32).reshape(1, -1)      # onset cells per step of the texture song, its segments joined
    return Steering(n=args.best_of, per=per_song, chord=rep(chd), mask=rep(mask), bass_relative=bool(args.score_bass_relative), onsets=onsets, **steer)


def autoreg_halves(v: torch.Tensor) -> torch.Tensor:
    """``[B, C, H, W]`` -> ``[2B, C, H/2, W]``: the segments cut into the halves ``--autoreg`` returns, in its order"""
    B, C, H, W = v.shape
    return v.reshape(B, C, 2, H // 2, W).permute(0, 2, 1, 3, 4).reshape(2 * B, C, H // 2, W)


def score_songs(gen: torch.Tensor, chd, mask, args, txt_prmat=None):
    """``--score`` on this rank's songs where they live: ``gen`` ``[n, B, C, H, W]`` (``[n, 2B, C, H/2, W]`` with ``--autoreg``) against the
    run's chords ``chd [B, 32, 36]`` (``None``: the chord-free numbers), of the cells ``mask [B, C, H, W]`` marks as invented when inpainting.
    Returns the per-song counters ``[n, 16]`` int32 (a song's segments summed) and, with ``txt_prmat`` ``[B, H, W]`` (the texture song of a
    chord+txt model), ``texture_fit`` per song, float64 ``[n]``, else ``None``.  Two launches at most, no host synchronisation."""
    n, per = gen.shape[0], gen.shape[1]
    if n == 0:
        return (torch.empty(0, _lib.ROLL_NCOUNT, dtype=torch.int32, device=gen.device),
                None if txt_prmat is None else torch.empty(0, dtype=torch.float64, device=gen.device))
    rep = lambda v: None if v is None else v.unsqueeze(0).expand(n, *v.shape)
    if mask is not None and args.autoreg:
        mask = autoreg_halves(mask)
    st = pfscore.roll_stats(gen, rep(chd), rep(mask), bass_relative=args.score_bass_relative).songs(per)
    if txt_prmat is None:
        return st.counters, None
    onset = (txt_prmat > 0).float()
    img = torch.stack([onset, torch.zeros_like(onset)], dim=1)                      # the texture song as an image of onsets alone
    ref = pfscore.roll_stats(autoreg_halves(img) if args.autoreg else img).songs(per)
    ref = pfscore.RollStats(ref.counters.expand(n, -1), ref.chroma.expand(n, -1, -1), ref.onsets.expand(n, -1))
    return st.counters, pfscore.texture_fit(st, ref)


def score_line(c: dict) -> str:
    return (f"chord_f1 {c['chord_f1']:.4f}  chord_fit {c['chord_fit']:.4f}  chord_cover {c['chord_cover']:.4f}  bass_fit {c['bass_fit']:.4f}  "
            f"integrity {c['integrity']:.4f}  onsets {c['counters']['N_ONSET']}" + (f"  texture_fit {c['texture_fit']:.4f}" if "texture_fit" in c else ""))


def recognizing(args) -> bool:
    """Whether the run recognises chords: ``--score_chords``, or a ranking that needs them"""
    return bool(getattr(args, "score_chords", False)) or (getattr(args, "best_of", 1) > 1 and getattr(args, "rank_by", "chord") == "extracted")


def recognize_songs(gen: torch.Tensor, chd, args):
    """``--score_chords`` on this rank's songs where they live: ``gen`` as in ``score_songs``, every song its ``gen.shape[1]`` images on one
    time axis, against the run's chords ``chd [B, 32, 36]`` (``None``: labels only).  Returns the counters ``[n, 8]`` and the labels
    ``[n, beats]``, both int32.  One launch, no host synchronisation."""
    n, per, steps = gen.shape[0], gen.shape[1], gen.shape[-2]
    beats = per * steps // 4
    if steps % 16 != 0 or beats > _lib.CHORDREC_MAX_BEATS:
        raise SystemExit(f"--score_chords: songs of {per} image(s) of {steps} steps: the recogniser takes whole bars of 16 steps and at most "
                         f"{_lib.CHORDREC_MAX_BEATS} beats per song")
    if n == 0:
        return (torch.empty(0, _lib.CHORDREC_NCOUNT, dtype=torch.int32, device=gen.device), torch.empty(0, beats, dtype=torch.int32, device=gen.device))
    rec = pfchordrec.recognize_rolls(gen, per, None if chd is None else chd.unsqueeze(0).expand(n, *chd.shape),
                                     bass_relative=args.score_bass_relative)
    return rec.counters, rec.labels


def recognized_report(counters: torch.Tensor, labels: torch.Tensor) -> list:
    """Per song: the five scores, the named counters and the label names (``ChordRecognition.report`` on gathered tensors)"""
    z = counters.new_zeros(0)
    return pfchordrec.ChordRecognition(labels, z, z, counters, z, z, z).report()


def chords_line(r: dict) -> str:
    runs = []
    for name in r["labels"]:
        if runs and runs[-1][0] == name:
            runs[-1][1] += 1
        else:
            runs.append([name, 1])
    return ("  ".join(f"{k} {r[k]:.4f}" for k in pfchordrec.SCORES) + "  " + " ".join(f"{k} {v}" for k, v in r["counters"].items())
            + "  chords: " + " ".join(f"{name}*{n}" if n > 1 else name for name, n in runs))


def load_novelty_corpus(args):
    """``--novelty_corpus``: the corpus file, or ``None`` without the flag.  A corpus this run cannot be compared with is a ``SystemExit``:
    windows of another size than the 128 steps of an image, or cells rounded by another rule than the run's (``v > 0.5``)."""
    path = getattr(args, "novelty_corpus", None)
    if not path:
        return None
    try:
        corpus = pfrollmatch.Corpus.load(path)
    except (OSError, ValueError, KeyError) as e:
        raise SystemExit(f"--novelty_corpus {path}: {e}")
    if corpus.steps != 128:
        raise SystemExit(f"--novelty_corpus {path}: windows of {corpus.steps} steps; a generated image has 128 (rebuild the corpus)")
    if corpus.custom_round:
        raise SystemExit(f"--novelty_corpus {path}: built with --custom_round, this run rounds by v > 0.5 (rebuild the corpus without it)")
    return corpus


def novelty_songs(gen: torch.Tensor, corpus, args):
    """``--novelty_corpus`` on this rank's songs where they live: ``gen`` as in ``score_songs``; every song's rows are cut into windows of
    128 steps (an image each; the two halves of ``--autoreg`` together) and matched against the corpus.  Returns ``copy_score`` float64
    ``[n]`` and ``pick`` int32 ``[n, 3]`` (window, shift, image of the song's best match).  No host synchronisation."""
    n = gen.shape[0]
    if n == 0:
        return torch.empty(0, dtype=torch.float64, device=gen.device), torch.empty(0, 3, dtype=torch.int32, device=gen.device)
    m = pfrollmatch.nearest(gen, corpus, args.novelty_shifts, args.novelty_topk, args.novelty_plane)
    return m.song_best(gen.shape[1] * gen.shape[-2] // corpus.steps)


def novelty_text(c: dict) -> str:
    w = c["nearest"]
    return f"copy_score {c['copy_score']:.4f}" + ("" if w is None else f" (nearest {w['song']} bar {w['bar']} shift {w['shift']:+d})")


def edit_song(model, params, args, image, cond, cond_tgt, cond_mid, cond_mid_tgt, scale, seed: int, say=print, score_chords=None) -> int:
    """``--edit``: the condition song's own image through ``Experiments.edit``; writes ``<stamp>.mid`` / ``.npy`` with ``_edit<K>`` in the
    stamp and prints the largest relative residual of the last iterate over all steps (and, with ``--edit_roundtrip``, how far the repaint
    under the song's own condition lands from it).  ``score_chords``: ``--score`` - the (source, target) chords ``[B, 32, 36]``; chord_f1 of the
    source image and of the edited one against each is printed and written to ``<stamp>_score.json`` (the edit took if the edited image
    scores higher on the target chords than on the source's)."""
    n = min(cond.shape[0], cond_tgt.shape[0], image.shape[0])
    cut = lambda v: None if v is None else v[:n].contiguous()
    sampler, t_idx = make_sampler(model, args, seed, 0)
    expmt = Experiments(params.model_name, params, sampler, t_idx=t_idx)
    depth = t_idx if args.edit_depth is None else args.edit_depth
    say(f"editing {n} segment(s): {depth + 1} upward steps x {args.edit_iters} iterates at scale "
        f"{scale if args.edit_invert_scale is None else args.edit_invert_scale}, then {depth + 1} steps down at uncond_scale = {scale}")
    orig = cut(image).float()
    res = expmt.edit(orig, cut(cond), cut(cond_tgt), scale, iters=args.edit_iters, depth=depth, invert_scale=args.edit_invert_scale,
                     cond_mid_src=cut(cond_mid), cond_mid_tgt=cut(cond_mid_tgt), joint=args.joint, blend=args.joint_blend,
                     roundtrip=args.edit_roundtrip)
    gen, rec = res if args.edit_roundtrip else (res, None)
    if not bool(torch.isfinite(gen).all()):
        raise SystemExit(f"non-finite values in the edited piano roll (precision {model.ldm.eps_model.precision})")
    last = sampler.last_inversion.residuals()[:, -1]
    say(f"inversion: largest relative residual of the last iterate over all steps: {float(np.nanmax(last)):.3e}")
    if rec is not None:
        differ = int(((rec > 0.5) != (orig > 0.5)).sum())
        say(f"round trip: max |x - x_rec| = {float((rec - orig).abs().max()):.3e}, note cells > 0.5 that differ: {differ} of {orig.numel()}")
    os.makedirs(args.output_dir, exist_ok=True)
    stamp = os.path.join(args.output_dir, expmt._stamp(scale, False, f"_edit{args.edit_iters}", args.joint_blend if args.joint else None))
    np.save(stamp + ".npy", gen.cpu().numpy())
    if rec is not None:
        np.save(stamp + "_roundtrip.npy", rec.cpu().numpy())
    midi.prmat2c_to_midi_file(gen, stamp + ".mid")
    say(f"edited song: piano_roll {tuple(gen.shape)}  onsets>0.5: {int((gen[:, 0] > 0.5).sum())}  -> {stamp}.mid")
    if score_chords is not None:
        doc = {"bass_relative": bool(args.score_bass_relative), "segments": n}
        for img_name, img in (("source", orig), ("edited", gen)):
            for chd_name, c in zip(("source_chords", "target_chords"), score_chords):
                doc[f"{img_name}_on_{chd_name}"] = pfscore.roll_stats(img, c[:n], bass_relative=args.score_bass_relative).songs(n).report()[0]
        f1 = lambda k: repr(doc[k]["chord_f1"])
        say(f"edit score (chord_f1): source image on source chords {f1('source_on_source_chords')}, on target chords {f1('source_on_target_chords')}; "
            f"edited image on source chords {f1('edited_on_source_chords')}, on target chords {f1('edited_on_target_chords')}")
        if recognizing(args):
            for img_name, img in (("source", orig), ("edited", gen)):
                for chd_name, c in zip(("source_chords", "target_chords"), score_chords):
                    cnt, lab = recognize_songs(img.unsqueeze(0), c[:n], args)
                    doc[f"{img_name}_on_{chd_name}"]["recognized"] = recognized_report(cnt, lab)[0]
            acc = lambda k: repr(doc[k]["recognized"]["chord_acc"])
            say(f"edit score (chord_acc): source image on source chords {acc('source_on_source_chords')}, on target chords "
                f"{acc('source_on_target_chords')}; edited image on source chords {acc('edited_on_source_chords')}, on target chords "
                f"{acc('edited_on_target_chords')}")
        corpus = load_novelty_corpus(args)
        if corpus is not None:                                   # the whole song is one candidate: source and edited image
            for img_name, img in (("source", orig), ("edited", gen)):
                doc[f"{img_name}_novelty"] = pfrollmatch.songs_report(*novelty_songs(img.unsqueeze(0), corpus, args), corpus)[0]
            say(f"edit score (novelty): source image {novelty_text(doc['source_novelty'])}; edited image {novelty_text(doc['edited_novelty'])}")
        with open(stamp + "_score.json", "w") as f:
            json.dump(doc, f, indent=1)
    return 0


def morph_songs(model, params, args, image_a, image_b, cond_a, cond_b, cond_mid_a, cond_mid_b, scale, seed: int, say=print,
                score_chords=None) -> int:
    """``--morph``: the path from song A to song B through ``Experiments.morph``; writes ``<stamp>_morph.npy`` ``[K, B, 2, H, W]``, one
    ``<stamp>_morph_<k>.mid`` per frame and ``<stamp>_morph.mid`` with the frames one after the other, and prints the largest relative
    residual of the inversions' last iterate and the angle between the two end noises per row.  Without the images the path runs between
    two fresh noise draws.  ``score_chords``: ``--score`` - (A's, B's) chords ``[B, 32, 36]``; chord_f1 of every frame against each is printed
    and written to ``<stamp>_score.json`` (the crossover is where the second column overtakes the first)."""
    n = min(cond_a.shape[0], cond_b.shape[0], *(v.shape[0] for v in (image_a, image_b) if v is not None))
    if any(v.shape[0] != n for v in (cond_a, cond_b, image_a, image_b) if v is not None):
        say(f"morph: both songs cut to {n} segment(s), the shorter one's")
    cut = lambda v: None if v is None else v[:n].contiguous()
    sampler, t_idx = make_sampler(model, args, seed, 0)
    expmt = Experiments(params.model_name, params, sampler, t_idx=t_idx)
    depth = t_idx if args.morph_depth is None else args.morph_depth
    K = args.morph_frames
    if image_a is None:
        say(f"morphing {n} segment(s) between two noise draws: {K} frames x {depth + 1} steps down at uncond_scale = {scale}")
    else:
        say(f"morphing {n} segment(s): {depth + 1} upward steps x {args.morph_iters} iterates on both songs, {K} frames ({args.morph_ease}, "
            f"conditions: {args.morph_cond}), then {depth + 1} steps down at uncond_scale = {scale}")
    gen = expmt.morph(cut(image_a), cut(cond_a), cut(image_b), cut(cond_b), K, scale, iters=args.morph_iters, depth=depth, ease=args.morph_ease,
                      cond_how=args.morph_cond, joint=args.joint, blend=args.joint_blend, cond_mid_a=cut(cond_mid_a), cond_mid_b=cut(cond_mid_b))
    if not bool(torch.isfinite(gen).all()):
        raise SystemExit(f"non-finite values in the morphed piano rolls (precision {model.ldm.eps_model.precision})")
    rec = sampler.last_morph
    if rec.inversion is not None:
        say(f"inversion: largest relative residual of the last iterate over all steps: {float(np.nanmax(rec.inversion.residuals()[:, -1])):.3e}")
    say("angle between the two end noises per " + ("song canvas" if args.joint else "segment") + " (radians): "
        + ", ".join(f"{v:.4f}" for v in rec.angles().tolist()))
    os.makedirs(args.output_dir, exist_ok=True)
    stamp = os.path.join(args.output_dir, expmt._stamp(scale, False, "", args.joint_blend if args.joint else None))
    np.save(stamp + "_morph.npy", gen.cpu().numpy())
    for k in range(K):
        midi.prmat2c_to_midi_file(gen[k], f"{stamp}_morph_{k}.mid")
    midi.prmat2c_to_midi_file(gen.reshape(K * n, *gen.shape[2:]), stamp + "_morph.mid")
    say(f"morph: {K} frames, piano_roll {tuple(gen.shape)}  onsets>0.5 per frame: {[int((gen[k][:, 0] > 0.5).sum()) for k in range(K)]}  "
        f"-> {stamp}_morph.mid, {stamp}_morph_<k>.mid")
    if score_chords is not None:
        doc = {"bass_relative": bool(args.score_bass_relative), "segments": n, "frames": K, "fractions": [float(t) for t in rec.fractions]}
        flat = gen.reshape(K * n, *gen.shape[2:])
        for name, c in zip(("chord_f1_on_a", "chord_f1_on_b"), score_chords):
            rep = pfscore.roll_stats(flat, c[:n].repeat(K, 1, 1), bass_relative=args.score_bass_relative).songs(n).report()
            doc[name] = [r["chord_f1"] for r in rep]
        if recognizing(args):
            for name, c in zip(("chord_acc_on_a", "chord_acc_on_b"), score_chords):
                doc[name] = [r["chord_acc"] for r in recognized_report(*recognize_songs(gen, c[:n], args))]
            doc["recognized"] = [r["labels"] for r in recognized_report(*recognize_songs(gen, None, args))]
        corpus = load_novelty_corpus(args)
        if corpus is not None:                                   # every frame is a song of n images
            doc["novelty"] = pfrollmatch.songs_report(*novelty_songs(gen, corpus, args), corpus)
        if getattr(args, "diversity", False):
            pw = pfrollmatch.pairwise(gen, segments=n, plane=args.novelty_plane)
            doc["nearest_other"], doc["diversity"] = pw["nearest_other"].tolist(), pw["diversity"]
            say(f"diversity of the {K} frames {doc['diversity']:.4f} (nearest_other per frame: " + ", ".join(f"{v:.4f}" for v in doc["nearest_other"]) + ")")
        for k in range(K):
            if corpus is not None:
                say(f"frame {k} novelty: {novelty_text(doc['novelty'][k])}")
            say(f"frame {k} (t = {rec.fractions[k]:.3f}) chord_f1: on A's chords {doc['chord_f1_on_a'][k]:.4f}, on B's chords {doc['chord_f1_on_b'][k]:.4f}"
                + (f"; chord_acc: on A's chords {doc['chord_acc_on_a'][k]:.4f}, on B's chords {doc['chord_acc_on_b'][k]:.4f}" if recognizing(args) else ""))
        with open(stamp + "_score.json", "w") as f:
            json.dump(doc, f, indent=1)
        say(f"scores -> {stamp}_score.json")
    return 0


def main(argv=None):
    from . import dist as pfdist
    args = make_parser().parse_args(argv)
    if args.dpm and args.ddim:
        raise SystemExit("--dpm and --ddim name two different samplers: give one of them")
    check_dpm_eta(args)
    check_guidance_args(args)                              # what the flags alone decide, before anything else
    check_threshold_args(args)
    check_edit_args(args)
    check_morph_args(args)
    check_score_args(args)
    check_steer_args(args)
    if not torch.cuda.is_available():
        raise SystemExit("inference_sdf needs an AMD GPU (no CPU fallback on this path)")
    rank, world, _ = pfdist.init_from_env()
    say = print if rank == 0 else (lambda *a, **k: None)
    if args.seed is not None:
        seed = args.seed
    else:
        # the reference seeds only on request (inference_sdf.py:510-514) and is otherwise random; the counter-based
        # generator needs SOME key, so draw one, share it across ranks and print it for reproducibility
        seed = pfdist.broadcast_int(int.from_bytes(os.urandom(4), "little"))
        say(f"seed: {seed} (pass --seed {seed} to reproduce)")
    torch.manual_seed(seed); np.random.seed(seed % (2 ** 32)); random.seed(seed)

    if args.params_preset is not None:
        params = preset(args.params_preset)
    else:
        if args.chkpt_path is None and args.custom_params_path is None:
            raise SystemExit("give --chkpt_path, --custom_params_path or --params_preset")
        try:
            params = load_params(find_params(args.chkpt_path or ".", args.custom_params_path))
        except FileNotFoundError:
            # extension: a Lightning checkpoint carries its own params (lightning_learner.py:13 save_hyperparameters)
            if not (args.chkpt_path or "").endswith(".ckpt"):
                raise
            from .checkpoint import load_lightning_ckpt
            saved = load_lightning_ckpt(args.chkpt_path)[1]
            if saved is None:
                raise
            params = Params(saved)
            params.setdefault("cond_mode", "cond")
            params.setdefault("use_enc", True)
    say(f"model_label: {params.model_name}")
    dual = wants_dual_guidance(args, params.cond_type)     # (refusals before any weight is loaded)
    editing = check_edit_args(args, params.cond_type, world)
    morphing = check_morph_args(args, params.cond_type, world)
    scoring = check_score_args(args, params.cond_type)
    steer = check_steer_args(args, params.cond_type)
    if steer is not None and (morphing or editing):
        raise SystemExit("--steer belongs to --best_of, which --edit and --morph do not take")
    if morphing and params.get("concat_blurry", False):
        raise SystemExit("--morph does not cover the concat_blurry variant (its blurred image describes one song, a frame lies between two)")
    if editing and params.get("concat_blurry", False):
        raise SystemExit("--edit does not cover the concat_blurry variant (its blurred image describes the song being changed)")
    try:
        model = load_model(params, args, rank, world)
    except SystemExit as e:
        if args.precision != "auto-f16x3":
            raise
        # the fp16-split library refused the checkpoint (a weight beyond its packing's range): the exact mode of the default library instead
        say(f"f16x3 not available for this checkpoint ({e}); loading it into the default library, precision f32")
        import copy
        args = copy.copy(args)
        args.precision = "f32"
        model = load_model(params, args, rank, world)

    length = args.length
    # prmat2c_cond: the CONDITION song's image (what concat_blurry blurs, ref:inference_sdf.py:797-803 uses `prmat2c`);
    # prmat2c_inp: the song to inpaint (`prmat2c_inp`, :565-591).  Two variables, as in the reference.
    chd = prmat = prmat2c_cond = prmat2c_inp = pnotree = None
    cond_is_dummy = False
    def song_from_midi(path, tag):
        # ref:inference_sdf.py:606-612 - quantise the file, extract its chords (written next to the outputs, as the reference's exp/*.out:
        # by rank 0 only - every rank extracts the same labels and keeps them in memory)
        from . import midi_to_data
        if rank == 0:
            os.makedirs(args.output_dir, exist_ok=True)
        data = midi_to_data.get_data_for_single_midi(path, os.path.join(args.output_dir, f"chords_extracted{tag}.out") if rank == 0 else None)
        if data is None:
            raise SystemExit(f"{path}: a barline does not fall on the 16th-note grid (get_downbeat_pos_and_filter)")
        return datasample.DataSample(data).get_whole_song_data()

    def song_from_dataset(name, index, use_track=(0, 1, 2)):
        # ref:inference_sdf.py:95-118 - a song of the validation half of the dataset's split (parity unpinned: the datasets are not shipped)
        try:
            sample, fn = datasample.choose_song_from_val_dl(name, index, use_track, args.dataset_dir, args.split_dir)
        except FileNotFoundError as e:
            raise SystemExit(f"--from_dataset {name}: {e} (give --dataset_dir / --split_dir)")
        return sample.get_whole_song_data(), fn

    def need_index(flag, value):
        # choose_song_from_val_dl asks on stdin when no index is given (ref:inference_sdf.py:95-118): under a multi-rank launch every
        # rank would block on input() - the index has to come from the command line there
        if world > 1 and value is None:
            raise SystemExit(f"{flag} is required when running on more than one rank (no interactive song choice under torchrun)")
        return value

    inp_from_midi = None
    if args.inpaint_type is not None and args.inpaint_from_midi is not None:    # :569-575
        inp_from_midi = song_from_midi(args.inpaint_from_midi, "_inpaint")[0].to(_dev())
        say(f"Inpainting midi file: {args.inpaint_from_midi}")
    elif args.inpaint_type is not None and args.inpaint_from_dataset is not None:   # :576-590
        tracks = [int(v) for v in args.inpaint_pop909_use_track.split(",")] if args.inpaint_pop909_use_track else [0, 1, 2]
        (p2c, _, _, _), fn = song_from_dataset(args.inpaint_from_dataset, need_index("--inpaint_song_index", args.inpaint_song_index), tracks)
        inp_from_midi = p2c.to(_dev())
        say(f"Inpainting midi file: {fn}")
    if args.uncond_scale != 0.0 and (args.from_midi is not None or args.from_dataset is not None):
        # the reference's order (:604-624): a MIDI file wins over a dataset song when both are given
        if args.from_midi is not None:
            p2c, pnotree, chd, prmat = song_from_midi(args.from_midi, "")
            fn = args.from_midi
        else:
            if args.from_dataset == "musicalion" and "chord" in params.cond_type.split("+"):
                raise SystemExit("--from_dataset musicalion has no chord track (ref:inference_sdf.py:620 asserts cond_type != 'chord'; "
                                 "a chord+txt model would receive chd = None)")
            (p2c, pnotree, chd, prmat), fn = song_from_dataset(args.from_dataset, need_index("--song_index", args.song_index))
        chd = None if chd is None else chd.to(_dev())
        prmat, prmat2c_cond, pnotree = prmat.to(_dev()), p2c.to(_dev()), pnotree.to(_dev())
        say(f"using the {params.cond_type.split('+')[0]} of midi file: {fn}")
        if params.cond_type == "chord+txt":                                       # texture from a second song (:627-641)
            if args.from_midi2 is not None:
                prmat = song_from_midi(args.from_midi2, "")[3].to(_dev())
                say(f"using the txt of midi file: {args.from_midi2}")
            elif args.from_dataset is not None:
                (_, _, _, prmat2), fn2 = song_from_dataset(args.from_dataset, need_index("--song_index2", args.song_index2))
                prmat = prmat2.to(_dev())
                say(f"using the txt of midi file: {fn2}")
            # else (an extension; the reference raises NotImplementedError): chords and texture both from --from_midi
    elif args.from_song_npz is not None:
        p2c, pnotree, chd, prmat = datasample.DataSample.from_npz(args.from_song_npz).get_whole_song_data()
        chd, prmat, prmat2c_cond, pnotree = chd.to(_dev()), prmat.to(_dev()), p2c.to(_dev()), pnotree.to(_dev())
    elif args.uncond_scale == 0.0 and args.cond_npz is None and not args.synthetic:
        if length <= 0 and inp_from_midi is not None:
            length = inp_from_midi.shape[0]            # :596-597
        if length <= 0:
            raise SystemExit("--length is required for unconditional generation")
        prmat2c_cond, pnotree, chd, prmat = dummy_cond_input(length, params)   # zeros: what an unconditional concat_blurry model blurs
        cond_is_dummy = True
    elif args.cond_npz is not None:
        z = np.load(args.cond_npz)
        chd = torch.from_numpy(z["chord"]).float().to(_dev()) if "chord" in z else None
        prmat = torch.from_numpy(z["prmat"]).float().to(_dev()) if "prmat" in z else None
        prmat2c_cond = torch.from_numpy(z["prmat2c"]).float().to(_dev()) if "prmat2c" in z else None
        pnotree = torch.from_numpy(z["pnotree"]).long().to(_dev()) if "pnotree" in z else None
    elif args.synthetic:
        n = length if length > 0 else 1
        chd = torch.from_numpy(synth.chords(n, seed + 100)).to(_dev())
        prmat = torch.from_numpy(synth.prmat(n, seed + 200)).to(_dev())
        if params.cond_type == "pnotree":
            pnotree = torch.from_numpy(synth.pnotree(n, seed + 300)).to(_dev())
    else:
        raise SystemExit("no condition source: use --from_midi, --from_song_npz, --cond_npz, --synthetic or --uncond_scale 0 --length N")

    if params.cond_type == "pnotree" and pnotree is None:
        raise SystemExit("cond_type pnotree needs the piano-tree grid: --from_midi, --from_song_npz, pnotree in --cond_npz or --synthetic")
    if args.polydis and rank == 0:
        write_polydis(args, chd, prmat, seed, say)
    cond, cond_mid = encode_conditions(model, params, chd, prmat, args.autoreg or args.joint, pnotree=pnotree)   # --joint: the same two streams
    # the guidance scale every later stage passes on unchanged: the float, or the two scales with the chord part's width as just concatenated
    scale = dual_scale(args, model.cond_split) if dual else args.uncond_scale
    if params.cond_type == "pnotree" and rank == 0 and not args.no_pnotree_recon:
        write_pnotree_recon(model, args, cond, say)
    cond_tgt = cond_mid_tgt = chd_tgt = None
    if editing:
        # the song's own condition is the source; the target is the same condition with the chords replaced
        if chd is None or prmat2c_cond is None or cond_is_dummy:
            raise SystemExit("--edit needs the song to edit with its chords: --from_midi, --from_dataset, --from_song_npz, or chord and prmat2c in --cond_npz")
        if args.edit_chord_shift is not None:
            chd_tgt = shift_chords(chd, args.edit_chord_shift)
        else:
            chd_tgt = song_from_midi(args.edit_chords_from_midi, "_edit")[2].to(_dev())
            say(f"target chords from midi file: {args.edit_chords_from_midi}")
        n = min(chd.shape[0], chd_tgt.shape[0])
        cond_tgt, cond_mid_tgt = encode_conditions(model, params, chd_tgt[:n], prmat, args.joint, pnotree=pnotree)
    cond_b = cond_mid_b = chd_b = image_b = None
    if morphing:
        # song B: its own chords (and texture, where it brings one), encoded like song A's
        prmat_b, pnotree_b = prmat, pnotree
        if args.morph_to_midi is not None:
            image_b, pnotree_b, chd_b, prmat_b = (v.to(_dev()) for v in song_from_midi(args.morph_to_midi, "_morph"))
            say(f"morphing to midi file: {args.morph_to_midi}")
        elif args.morph_to_song_index is not None:
            (image_b, pnotree_b, chd_b, prmat_b), fn_b = song_from_dataset(args.from_dataset, args.morph_to_song_index)
            image_b, pnotree_b, chd_b, prmat_b = (v.to(_dev()) for v in (image_b, pnotree_b, chd_b, prmat_b))
            say(f"morphing to midi file: {fn_b}")
        elif args.morph_to_npz is not None:
            with np.load(args.morph_to_npz) as zb:
                if "chord" not in zb or "prmat2c" not in zb:
                    raise SystemExit(f"--morph_to_npz {args.morph_to_npz}: needs the arrays chord [B,32,36] and prmat2c [B,2,128,128]")
                chd_b, image_b = (torch.from_numpy(zb[k]).float().to(_dev()) for k in ("chord", "prmat2c"))
                prmat_b = torch.from_numpy(zb["prmat"]).float().to(_dev()) if "prmat" in zb else prmat
        else:                  # --synthetic: a second draw of the synthetic conditions, no images
            n_b = cond.shape[0]
            chd_b = torch.from_numpy(synth.chords(n_b, seed + 101)).to(_dev())
            prmat_b = torch.from_numpy(synth.prmat(n_b, seed + 201)).to(_dev())
            pnotree_b = torch.from_numpy(synth.pnotree(n_b, seed + 301)).to(_dev()) if params.cond_type == "pnotree" else None
        if image_b is not None and (chd is None or prmat2c_cond is None):
            raise SystemExit("--morph needs song A with its chords and its image: --from_midi, --from_dataset, --from_song_npz, or chord and prmat2c in --cond_npz")
        cond_b, cond_mid_b = encode_conditions(model, params, chd_b, prmat_b, args.joint, pnotree=pnotree_b)
    if params.cond_mode == "uncond":
        cond = -torch.ones_like(cond)
    if length > 0:
        cond_b = None if cond_b is None else cond_b[:length]
        cond_mid_b = None if cond_mid_b is None else cond_mid_b[:length]
        cond = cond[:length]
        cond_mid = cond_mid[:length] if cond_mid is not None else None
        cond_tgt = None if cond_tgt is None else cond_tgt[:length]
        cond_mid_tgt = None if cond_mid_tgt is None else cond_mid_tgt[:length]
    orig = mask = None
    # the image to inpaint: --inpaint_from_midi, else (an extension of the reference, whose dataset branches are absent here) the condition song
    prmat2c_inp = inp_from_midi if inp_from_midi is not None else (None if cond_is_dummy else prmat2c_cond)
    if args.inpaint_type is not None:
        if prmat2c_inp is None:
            raise SystemExit("--inpaint_type needs the image to inpaint: --inpaint_from_midi, prmat2c in --cond_npz, or a --from_midi / --from_song_npz song")
        n = min(cond.shape[0], prmat2c_inp.shape[0])
        cond, orig = cond[:n], prmat2c_inp[:n]
        cond_mid = None if cond_mid is None else cond_mid[:n]
        bars = [int(v) for v in args.bar_list.split(",")] if args.bar_list else None
        mask = get_mask(orig, args.inpaint_type, bars).to(orig.device)

    cond_concat = None
    if params.get("concat_blurry", False):
        # inference_sdf.py:797-803 - the denoiser of this variant takes cat([x, blurry image], 1)
        if prmat2c_cond is None:
            raise SystemExit("params.concat_blurry needs the condition song's image to blur: --from_midi, --from_song_npz, prmat2c in --cond_npz, "
                             "or --uncond_scale 0 --length N (zeros)")
        cond_concat = get_blurry_image(prmat2c_cond[:cond.shape[0]], params.get("concat_ratio", 1 / 8))
        n = min(cond.shape[0], cond_concat.shape[0])
        cond, cond_concat = cond[:n], cond_concat[:n]
        cond_mid = None if cond_mid is None else cond_mid[:n]
        orig, mask = (None if v is None else v[:n] for v in (orig, mask))
    if args.precision in ("auto", "auto-f16x3"):
        def probe(mdl):
            split = mdl.ldm.eps_model.split_mode
            mode, ratio = pick_precision(mdl.ldm.eps_model, cond.reshape(-1, *cond.shape[-2:]), n_steps=params.n_steps, seed=seed)
            mode = ["f32", split][pfdist.broadcast_int(int(mode == split))]        # one decision for all ranks (rank 0's)
            mdl.ldm.eps_model.set_precision(mode)
            # printed by EVERY rank's log prefix owner (rank 0) and kept in the run's stamp: which arithmetic produced the files
            am = pick_precision.last_absmax
            say(f"precision: {mode} ({split} vs f32 on probe inputs: {ratio:.1e} of the output scale, threshold {PRECISION_PROBE_TOL:.0e}; "
                f"largest |activation| stored on the probe {am:.3g} = fp16 headroom x{65504.0 / am if am > 0 else float('inf'):.0f}"
                f"{', f16x3 needs x%g' % F16_HEADROOM_MIN if split == 'f16x3' else ''}); "
                "the probe is one evaluation on noise - for a run that must match the reference to its fp32 rounding, pass --precision f32")
            return mode
        if probe(model) == "f32" and args.precision == "auto":
            # bf16x3 does not hold this checkpoint to the contract: before paying 3x for the fp32 mode, try the fp16 split (22 mantissa bits per
            # product instead of 16, ~3 % slower than bf16x3) - the same weights loaded into the other build of the library, the same probe
            import copy
            args16 = copy.copy(args)
            args16.precision = "auto-f16x3"
            try:
                model16 = load_model(params, args16, rank, world)
            except SystemExit as e:      # e.g. a weight beyond the fp16 packing's range (load_model raises SystemExit on every rank)
                say(f"f16x3 not available for this checkpoint ({e}); staying with f32")
                model16 = None
            if model16 is not None and probe(model16) == "f16x3":
                model = model16
    else:
        model.ldm.eps_model.set_precision(args.precision)
    if morphing:
        return morph_songs(model, params, args, None if image_b is None else prmat2c_cond, image_b, cond, cond_b, cond_mid, cond_mid_b, scale, seed, say,
                           score_chords=(chd, chd_b) if scoring and chd is not None and chd_b is not None else None)
    if editing:
        return edit_song(model, params, args, prmat2c_cond, cond, cond_tgt, cond_mid, cond_mid_tgt, scale, seed, say,
                         score_chords=(chd, chd_tgt) if scoring else None)
    S, B = args.num_generate, cond.shape[0]
    S_all = S * args.best_of                        # --best_of N: N candidates per song kept, each a song of its own until the ranking
    say(f"generating {S} song(s) x {B} segment(s) with uncond_scale = {scale} on {world} GPU(s)")
    if args.best_of > 1:
        say(f"best of {args.best_of}: {S_all} candidates, the best {S} by {pfscore.RANK_BY[args.rank_by][0]} are kept")
    novelty_corpus = load_novelty_corpus(args) if scoring else None      # refused before the songs are generated, not after
    chd_steer = chd[:B] if chd is not None and not cond_is_dummy and "chord" in params.cond_type.split("+") else None
    if steer is not None and steer["reward"] in ("chord", "bass") and chd_steer is None:
        raise SystemExit(f"--steer_by {steer['reward']} needs the chords of the run, and this run has none")
    gen, expmt = generate_songs(model, params, args, cond, cond_mid, orig, mask, seed, rank, world, cond_concat=cond_concat, uncond_scale=scale,
                                steer=steer, chd=chd_steer, txt_prmat=prmat[:B] if params.cond_type == "chord+txt" and prmat is not None else None)
    if steer is not None:
        # the ranks hold whole groups (steer_shard): the end-of-run exchange moves groups of best_of candidates
        gather_rows = lambda v, total, r, w: pfdist.gather_rows(v.reshape(-1, args.best_of, *v.shape[1:]), S, r, w).reshape(total, *v.shape[1:])
        events = expmt.sampler.last_steering
        steer_doc = dict(steer, n=args.best_of, events=None if events is None else events.report(),
                         lineage=None if events is None else events.lineage().tolist(), groups=list(steer_shard(S, 1, rank, world)))
        steer_docs = pfdist.gather_objects(steer_doc, rank, world)
    else:
        gather_rows = pfdist.gather_rows
    counters = texture = None
    if scoring:
        # scored where the songs live, against the chords the run conditioned on (a model without a chord condition, or a run on the dummy
        # condition, gets the chord-free numbers); 64 bytes of counters per song travel beside the rows
        chd_score = chd[:B] if chd is not None and not cond_is_dummy and "chord" in params.cond_type.split("+") else None
        counters, texture = score_songs(gen, chd_score, mask, args, prmat[:B] if params.cond_type == "chord+txt" and prmat is not None else None)
        counters = gather_rows(counters, S_all, rank, world)
        texture = None if texture is None else gather_rows(texture, S_all, rank, world)
        if recognizing(args):
            rc_counters, rc_labels = (gather_rows(v, S_all, rank, world) for v in recognize_songs(gen, chd_score, args))
        if novelty_corpus is not None:
            nv_score, nv_pick = (gather_rows(v, S_all, rank, world) for v in novelty_songs(gen, novelty_corpus, args))
    gen = gather_rows(gen, S_all, rank, world)   # [S, ...] on every rank (131 KB per image; the only end-of-run exchange)
    if not bool(torch.isfinite(gen).all()):
        # the note threshold (> 0.5) would turn a NaN into silence: refuse instead.  The one known way to get here is an activation beyond
        # fp16's range in the f16x3 mode on a checkpoint the probe inputs did not exercise (include/pfhip.h pf_x3_element)
        mode = model.ldm.eps_model.precision
        raise SystemExit(f"non-finite values in the generated piano rolls (precision {mode})"
                         + ("; f16x3 overflows beyond 65504: rerun with --precision bf16x3 or f32" if mode == "f16x3" else ""))
    if rank == 0:
        os.makedirs(args.output_dir, exist_ok=True)
        stamps = []
        extra = "" if args.inpaint_type is None else f"_inp{args.repaint_n}_{args.inpaint_type}"
        order, cands = list(range(S)), None         # which candidate file i holds: itself, or with --best_of the one ranked i
        if scoring:
            cands = pfscore.report_of(counters, gen.shape[1] * gen.shape[-2])
            for c, t in zip(cands, [] if texture is None else texture.tolist()):
                c["texture_fit"] = t
            if recognizing(args):
                recog = recognized_report(rc_counters, rc_labels)
                for c, r in zip(cands, recog):
                    c.update({k: r[k] for k in pfchordrec.SCORES})
            if novelty_corpus is not None:
                for c, r in zip(cands, pfrollmatch.songs_report(nv_score, nv_pick, novelty_corpus)):
                    c.update(r)
            if args.best_of > 1:
                key, descending = pfscore.RANK_BY[args.rank_by]
                order = pfscore.rank([c[key] for c in cands], S, descending)
            score_stamp = os.path.join(args.output_dir, expmt._stamp(scale, args.autoreg, extra, args.joint_blend if args.joint else None))
        gen = gen[torch.tensor(order, device=gen.device)] if order != list(range(S_all)) else gen
        diversity = None
        if scoring and args.diversity:                           # of the kept songs, among themselves, whole images, no transposition
            diversity = pfrollmatch.pairwise(gen[:S], segments=gen.shape[1] * gen.shape[-2] // 128, plane=args.novelty_plane, steps=128)
        for i in range(S):
            stamp = os.path.join(args.output_dir, expmt._stamp(scale, args.autoreg, extra, args.joint_blend if args.joint else None)
                                 + (f"_{i}" if S > 1 else ""))
            stamps.append(stamp)
            np.save(stamp + ".npy", gen[i].cpu().numpy())
            # generated cells on their own track when inpainting (ref:inference_sdf.py:385-389)
            midi.prmat2c_to_midi_file(gen[i], stamp + ".mid", inp_mask=None if args.autoreg else mask)
            say(f"song {i}: piano_roll {tuple(gen[i].shape)}  onsets>0.5: {int((gen[i][:, 0] > 0.5).sum())}  -> {stamp}.mid")
            if scoring:
                say(f"song {i} score: {score_line(cands[order[i]])}" + (f"  {novelty_text(cands[order[i]])}" if novelty_corpus is not None else "")
                    + (f"  nearest_other {diversity['nearest_other'][i]:.4f}" if diversity is not None else "")
                    + (f"  (candidate {order[i]} of {S_all})" if args.best_of > 1 else ""))
                if recognizing(args):
                    say(f"song {i} chords: {chords_line(recog[order[i]])}")
        if scoring:
            doc = {"best_of": args.best_of, "rank_by": args.rank_by if args.best_of > 1 else None, "bass_relative": bool(args.score_bass_relative),
                   "chords": chd_score is not None, "masked": mask is not None, "steps": int(gen.shape[1] * gen.shape[-2]),
                   "songs": [dict(cands[order[i]], candidate=order[i], file=os.path.basename(stamps[i]) + ".npy") for i in range(S)],
                   "candidates": cands}
            if recognizing(args):
                doc["recognized"] = [dict(recog[order[i]], candidate=order[i]) for i in range(S)]
            if novelty_corpus is not None:
                doc["novelty"] = {"corpus": args.novelty_corpus, "windows": len(novelty_corpus), "shifts": args.novelty_shifts,
                                  "topk": args.novelty_topk, "plane": args.novelty_plane, "masked": False}
            if steer is not None:
                # per rank: the events of its groups (ESS, resample flags, u per group) and the lineage of its candidates; per kept song: the
                # start candidate it descends from
                lin = [a for d in steer_docs if d["lineage"] is not None for a in d["lineage"]]          # [group][particle], global group order
                doc["steer"] = {"by": steer["reward"], "lambda": steer["lam"], "every": steer["every"], "window": list(steer["window"]),
                                "ess": steer["ess"], "n": args.best_of,
                                **(dict(sampler="dpm", eta=float(args.dpm_eta)) if args.dpm else {}),      # (the stochastic 2M loop names itself)
                                "ranks": [dict(groups=d["groups"], events=d["events"]) for d in steer_docs],
                                "lineage": [dict(candidate=order[i], descends_from=(order[i] // args.best_of) * args.best_of
                                                 + lin[order[i] // args.best_of][order[i] % args.best_of]) for i in range(S)]}
            if diversity is not None:
                for i in range(S):
                    doc["songs"][i]["nearest_other"] = float(diversity["nearest_other"][i])
                doc["diversity"] = diversity["diversity"]
                say(f"diversity of the {S} kept song(s): {diversity['diversity']:.4f}")
            with open(score_stamp + "_score.json", "w") as f:
                json.dump(doc, f, indent=1)
            say(f"scores -> {score_stamp}_score.json")
        if args.polydis_recon:
            if params.cond_type in ("chord", "chord+txt") and args.inpaint_type is None and chd is not None:
                n_seg = min(chd.shape[0], prmat.shape[0]) if params.cond_type == "chord+txt" and prmat is not None else chd.shape[0]
                write_polydis_recon(args, [gen[i] for i in range(S)], stamps, chd[:min(n_seg, B)], say)
            else:
                say("--polydis_recon does nothing here: it applies to generation (not inpainting) with cond_type chord or chord+txt")
    pfdist.barrier()
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
