"""``Chord_8Bar`` (``models/model_chd_8bar.py``): the chord VAE whose encoder every ``sdf_chd8bar*`` model conditions on, forward only -
what the reference's learner logs as ``val/loss`` (``root`` / ``chroma`` / ``bass``) while it pretrains that encoder.

``get_loss_dict`` is three things on the device: the encoder's Normal (``pf_encoder_forward_dist``) and its ``rsample()``
(``pf_normal_rsample``), the teacher-forced decode (``ChordDecoder.forward_forced``) and the three cross-entropies
(``pf_chord_ce_rows``, per row in float64).  What the reference leaves to global generators is pinned as ``validate`` pins it: the
noise is draw ``draw`` of the library's counter-based generator under ``seed`` with the element index counted from ``elem_offset``;
the teacher-forcing coin flips come from Python's ``random`` in the reference's order, so a seeded ``random`` makes its choices.

No backward pass: this scores a checkpoint, it does not train one.
"""
from __future__ import annotations

import os
import random
from typing import Mapping, Optional

import numpy as np
import torch

from . import _lib
from .decoders import ChordDecoder
from .model_sdf import ChordEncoder

# params/chd_8bar.yaml: the model-defining keys and the teacher-forcing pair (high, low) of train/train_chd_8bar.py:15-16
CHD_8BAR = dict(model_name="chd_8bar", batch_size=128, tfr_chd=(0.5, 0.0), chd_n_step=32, chd_input_dim=36, chd_z_input_dim=512,
                chd_hidden_dim=512, chd_z_dim=512)


def teacher_forcing_rate(step, high: float = 0.7, low: float = 0.05) -> float:
    """``scheduled_sampling`` (``train/scheduler.py:6-11``): the rate ``TeacherForcingScheduler(high, low)`` hands out at global step ``step``."""
    i = step / (1000 * 40)
    x = 10 * (i - 0.5)
    z = 1 / (1 + np.exp(x))
    return float((high - low) * z + low)


def normal_rsample(mean: torch.Tensor, std: torch.Tensor, noise: Optional[torch.Tensor] = None, *, seed: int = 0, draw: int = 0,
                   elem_offset: int = 0, lib=None) -> torch.Tensor:
    """``Normal(mean, std).rsample()``: ``mean + std * noise`` as two rounded operations, in one launch.  ``noise=None``: element ``i``
    takes what ``pf_randn(seed, draw, elem_offset)`` writes at ``i``."""
    lib = lib or _lib.load()
    mean, std = mean.contiguous().float(), std.contiguous().float()
    assert mean.shape == std.shape and mean.is_cuda
    if noise is not None:
        noise = noise.to(device=mean.device, dtype=torch.float32).contiguous()
        assert noise.shape == mean.shape
    z = torch.empty_like(mean)
    _lib.check(lib.pf_normal_rsample(mean.data_ptr(), std.data_ptr(), _lib.ptr(noise), int(seed), int(draw), int(elem_offset), z.data_ptr(),
                                     z.numel(), _lib.current_stream()), "pf_normal_rsample", lib)
    return z


def chord_ce_rows(c: torch.Tensor, recon_root: torch.Tensor, recon_chroma: torch.Tensor, recon_bass: torch.Tensor, hits: bool = True, lib=None):
    """Per-row sums of the three cross-entropies (float64 ``[B, 3]``: root, chroma, bass) and, with ``hits``, the per-row counts of
    arg-maxes that equal their target (int32 ``[B, 3]``)."""
    lib = lib or _lib.load()
    B, n = recon_root.shape[0], recon_root.shape[1]
    assert tuple(c.shape) == (B, n, 36) and tuple(recon_root.shape) == (B, n, 12) and tuple(recon_bass.shape) == (B, n, 12)
    assert recon_chroma.numel() == B * n * 24
    dev = recon_root.device
    c = c.detach().to(device=dev, dtype=torch.float32).contiguous()
    r, ch, b = (t.detach().to(torch.float32).contiguous() for t in (recon_root, recon_chroma, recon_bass))
    ce = torch.empty(B, 3, dtype=torch.float64, device=dev)
    hit = torch.empty(B, 3, dtype=torch.int32, device=dev) if hits else None
    _lib.check(lib.pf_chord_ce_rows(r.data_ptr(), ch.data_ptr(), b.data_ptr(), c.data_ptr(), B, n, ce.data_ptr(), _lib.ptr(hit),
                                    _lib.current_stream()), "pf_chord_ce_rows", lib)
    return ce, hit


class Chord_8Bar:
    def __init__(self, chord_enc: ChordEncoder, chord_dec: ChordDecoder):
        if not getattr(chord_enc, "with_scale", False):
            raise ValueError("Chord_8Bar: the chord encoder must be created with with_scale=True (the loss samples its Normal)")
        self.chord_enc, self.chord_dec = chord_enc, chord_dec

    @classmethod
    def from_params(cls, params: Optional[Mapping] = None, device=None) -> "Chord_8Bar":
        """The modules of ``Chord8bar_TrainConfig`` (``train/train_chd_8bar.py:22-37``) at the sizes of ``params`` (default ``CHD_8BAR``)."""
        p = dict(CHD_8BAR, **(params or {}))
        enc = ChordEncoder(p["chd_input_dim"], p["chd_hidden_dim"], p["chd_z_dim"], device, with_scale=True)
        dec = ChordDecoder(p["chd_input_dim"], p["chd_z_input_dim"], p["chd_hidden_dim"], p["chd_z_dim"], p["chd_n_step"], device)
        return cls(enc, dec)

    @classmethod
    def load_trained(cls, chord_enc, chord_dec, model_dir) -> "Chord_8Bar":
        """``models/model_chd_8bar.py:14-19``: ``<model_dir>/weights.pt`` (``{"model": state_dict}``); a file path is read as it is, in
        either checkpoint format."""
        from .checkpoint import load_checkpoint
        path = str(model_dir)
        if os.path.isdir(path):
            path = os.path.join(path, "weights.pt")
        return cls(chord_enc, chord_dec).load_state_dict(load_checkpoint(path)[0])

    def load_state_dict(self, state: Mapping[str, object]) -> "Chord_8Bar":
        if "model" in state:
            state = state["model"]
        part = lambda name: {k[len(name) + 1:]: v for k, v in state.items() if k.split(".")[0] == name}
        enc, dec = part("chord_enc"), part("chord_dec")
        if not enc or not dec:
            raise RuntimeError("Chord_8Bar.load_state_dict: the state holds no chord_enc.* / chord_dec.* keys")
        self.chord_enc.load_state_dict(enc)
        self.chord_dec.load_state_dict(dec)
        return self

    def eval(self):
        return self

    def chord_loss(self, c, recon_root, recon_chroma, recon_bass, *, detail: bool = False) -> dict:
        """``models/model_chd_8bar.py:21-39``: the means of the three cross-entropies and their sum (float32 scalars on the device, as
        the reference returns them).  ``detail`` adds ``loss_rows`` (float64 ``[B, 3]``: every row's own means of root, chroma, bass),
        ``hit_rows`` (int32 ``[B, 3]``: correct arg-maxes out of ``n_step``, ``12 n_step``, ``n_step``) and ``acc`` (their batch rates)."""
        ce, hit = chord_ce_rows(c, recon_root, recon_chroma, recon_bass, hits=detail, lib=self.chord_dec._lib)
        B, n = recon_root.shape[0], recon_root.shape[1]
        count = torch.tensor([n, 12 * n, n], dtype=torch.float64, device=ce.device)
        rows = ce / count
        means = rows.sum(0) / B            # CrossEntropyLoss(reduction="mean") over the B * n (B * n * 12) items: every row has as many
        out = {"loss": (means[0] + means[1] + means[2]).float(), "root": means[0].float(), "chroma": means[1].float(), "bass": means[2].float()}
        if detail:
            out.update(loss_rows=rows, hit_rows=hit, acc=hit.sum(0).double() / (count * B), loss64=means[0] + means[1] + means[2])
        return out

    def get_loss_dict(self, batch, step, tfr_chd, *, detail: bool = False, feedback: str = "row", noise: Optional[torch.Tensor] = None,
                      seed: int = 0, draw: int = 0, elem_offset: int = 0) -> dict:
        """``models/model_chd_8bar.py:41-48`` on a reference-layout batch ``(_, _, chord, _)``: ``{"loss", "root", "chroma", "bass"}``.

        The ``n_step - 1`` teacher-forcing flips are ``random.random() < tfr_chd`` from Python's ``random``, drawn once per call in the
        reference's order - also at rate 0, as the reference draws them.  ``feedback``: ``"row"`` (every row decodes as a batch of one;
        invariant to how the batch is split) or ``"batch"`` (the reference's union token over the rows of this call, which is what its
        logged numbers contain at the logged batch size).  ``noise``: the ``eps`` of ``rsample`` as a tensor ``[B, z_dim]``, or ``None``
        for draw ``draw`` of the library's generator under ``seed``, row ``b`` at element ``elem_offset + b * z_dim``.
        ``detail`` adds ``loss_rows``, ``hit_rows``, ``acc``, ``loss64`` (``chord_loss``) and ``flips`` (the booleans used)."""
        _, _, chord, _ = batch
        mean, std = self.chord_enc.encode_dist(chord)
        z_chd = normal_rsample(mean, std, noise, seed=seed, draw=draw, elem_offset=elem_offset, lib=self.chord_dec._lib)
        flips = [random.random() < tfr_chd for _ in range(self.chord_dec.n_step - 1)]
        recon = self.chord_dec.forward_forced(z_chd, chord, flips, feedback)
        out = self.chord_loss(chord, *recon, detail=detail)
        if detail:
            out["flips"] = flips
        return out
