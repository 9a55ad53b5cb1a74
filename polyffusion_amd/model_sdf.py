"""Conditioning wrapper and frozen encoders (host mirrors backed by libpfhip.so).

* ``ChordEncoder`` / ``TextureEncoder``: constructor argument order of the reference modules
  (``dl_modules/chord_enc.py:6``, ``dl_modules/txt_enc.py:6``); ``encode_mean`` returns what the
  reference reads from them, ``forward(x).mean``.
* ``Polyffusion_SDF``: ``models/model_sdf.py`` - ``_encode_chord`` (:92-106), ``_encode_txt``
  (:153-164) and ``load_trained`` (:59-84; legacy ``.pt`` with ``{"model": state_dict}``).
* ``load_pretrained_chd_enc`` / ``load_pretrained_txt_enc``: the key-prefix remaps of
  ``utils.py:48-86`` (``chord_enc.`` / ``rhy_encoder.``).
* ``get_loss_dict`` (:185-234): the condition of a training batch and ``ldm.loss`` on it - what the reference's learner logs as
  ``val/loss``.
* ``PianoTreeDecoder`` / ``ChordDecoder`` (``decoders.py``), ``_decode_pnotree`` (:166-183), ``_decode_chord`` (:108-136) and
  ``load_pretrained_pnotree_enc_dec`` / ``load_pretrained_chd_enc_dec`` (``utils.py:19-69``).
"""
from __future__ import annotations

import random
from types import SimpleNamespace
from typing import Mapping, Optional

import torch

from . import _lib
from ._handle import ModelHandle
from .decoders import ChordDecoder, PianoTreeDecoder  # noqa: F401  (part of this module's surface, like the reference's dl_modules)
from .unet import LatentDiffusion


class _Encoder(ModelHandle):
    """A frozen encoder on the ``pf_encoder`` handle (weights: ModelHandle; no parameter table)."""
    PREFIX = "pf_encoder"
    KIND = -1

    def __init__(self, input_dim, emb_size, hidden_dim, z_dim, num_channel, device=None, with_scale=False):
        """``with_scale``: keep ``linear_var.*`` and produce the Normal's scale too (``encode_dist``; the Polydis encoders)."""
        self.hidden_dim, self.z_dim, self.with_scale = hidden_dim, z_dim, bool(with_scale)
        super().__init__(_lib.load(), self.KIND, input_dim, emb_size, hidden_dim, z_dim, num_channel, int(self.with_scale), device=device)

    def _fn(self, name: str):
        return super()._fn("create_dist" if name == "create" else name)   # pf_encoder_create is its with_scale = 0 case

    def _run(self, x: torch.Tensor, n_step: int, dist: bool = False):
        if self._blob_dev is None:
            raise RuntimeError("encoder weights not loaded")
        x = x.contiguous().float()
        B = x.shape[0]
        ws = self.workspace_for(self._lib.pf_encoder_workspace_bytes(self._h, B), x.device)
        mu = torch.empty(B, self.z_dim, dtype=torch.float32, device=x.device)
        if dist:
            scale = torch.empty(B, self.z_dim, dtype=torch.float32, device=x.device)
            self._check(self._lib.pf_encoder_forward_dist(self._h, x.data_ptr(), B, n_step, mu.data_ptr(), scale.data_ptr(), ws.data_ptr(),
                                                          ws.numel(), _lib.current_stream()), "pf_encoder_forward_dist")
            return mu, scale
        self._check(self._lib.pf_encoder_forward(self._h, x.data_ptr(), B, n_step, mu.data_ptr(), ws.data_ptr(), ws.numel(),
                                                 _lib.current_stream()), "pf_encoder_forward")
        return mu

    def forward(self, x):
        """Reference call shape: returns an object whose ``.mean`` is the encoder mean."""
        return SimpleNamespace(mean=self.encode_mean(x))

    __call__ = forward


class ChordEncoder(_Encoder):
    KIND = 0

    def __init__(self, input_dim, hidden_dim, z_dim, device=None, with_scale=False):
        super().__init__(input_dim, 0, hidden_dim, z_dim, 0, device, with_scale)

    def encode_mean(self, chord: torch.Tensor) -> torch.Tensor:  # [B,T,input_dim] -> [B,z]
        return self._run(chord, chord.shape[1])

    def encode_dist(self, chord: torch.Tensor):                  # -> (mean [B,z], scale [B,z]); needs with_scale
        return self._run(chord, chord.shape[1], dist=True)


class TextureEncoder(_Encoder):
    KIND = 1

    def __init__(self, emb_size, hidden_dim, z_dim, num_channel=10, device=None, with_scale=False):
        super().__init__(0, emb_size, hidden_dim, z_dim, num_channel, device, with_scale)

    def encode_mean(self, pr: torch.Tensor) -> torch.Tensor:  # [B,32,128] -> [B,z]
        assert tuple(pr.shape[1:]) == (32, 128), "texture encoder input must be [B,32,128]"
        return self._run(pr, 8)

    def encode_dist(self, pr: torch.Tensor):                   # -> (mean [B,z], scale [B,z]); needs with_scale
        assert tuple(pr.shape[1:]) == (32, 128), "texture encoder input must be [B,32,128]"
        return self._run(pr, 8, dist=True)


class PianoTreeEncoder(_Encoder):
    """``dl_modules/pianotree_enc.py:7-59`` (constructor keywords kept); ``forward`` returns ``(dist, None, lengths)`` so that the
    reference's ``self.pnotree_enc(seg)[0].mean`` (models/model_sdf.py:144) reads the same."""
    KIND = 2

    def __init__(self, max_simu_note=20, max_pitch=127, min_pitch=0, pitch_sos=128, pitch_eos=129, pitch_pad=130, dur_pad=2, dur_width=5,
                 num_step=32, note_emb_size=128, enc_notes_hid_size=256, enc_time_hid_size=512, z_size=512, device=None):
        if num_step != 32 or max_simu_note > 32:
            raise ValueError("PianoTreeEncoder: num_step must be 32 and max_simu_note at most 32")
        self.max_simu_note, self.pitch_pad, self.num_step = max_simu_note, pitch_pad, num_step
        pitch_range = max_pitch - min_pitch + 3
        if pitch_pad != pitch_range:
            raise ValueError("PianoTreeEncoder: pitch_pad must be the index right after the pitch classes (max_pitch - min_pitch + 3)")
        super().__init__(pitch_range + dur_width, note_emb_size, enc_time_hid_size, z_size, enc_notes_hid_size, device)

    def encode_mean(self, grid: torch.Tensor) -> torch.Tensor:   # [R,32,max_simu_note,6] integer grid -> [R,z]
        assert tuple(grid.shape[1:]) == (self.num_step, self.max_simu_note, 6), "pianotree grid must be [B,32,max_simu_note,6]"
        return self._run(grid.to(torch.float32), self.max_simu_note)

    def forward(self, grid):
        lengths = self.max_simu_note - (grid[:, :, :, 0] == self.pitch_pad).sum(dim=-1)
        return SimpleNamespace(mean=self.encode_mean(grid)), None, lengths.cpu()

    __call__ = forward


def _strip(state, part: str):
    if isinstance(state, (str, bytes)) or hasattr(state, "__fspath__"):   # a checkpoint path, like the reference's fpath argument
        from .checkpoint import load_checkpoint
        state = load_checkpoint(str(state))[0]
    if "model" in state:
        state = state["model"]
    return {".".join(k.split(".")[1:]): v for k, v in state.items() if k.split(".")[0] == part}


def load_pretrained_chd_enc(state: Mapping[str, object], input_dim, hidden_dim, z_dim, device=None) -> ChordEncoder:
    """utils.py:48-69: keep the ``chord_enc.`` keys of a chd_8bar checkpoint."""
    return ChordEncoder(input_dim, hidden_dim, z_dim, device).load_state_dict(_strip(state, "chord_enc"))


def load_pretrained_txt_enc(state: Mapping[str, object], emb_size, hidden_dim, z_dim, num_channel, device=None) -> TextureEncoder:
    """utils.py:72-86: keep the ``rhy_encoder.`` keys of a Polydis checkpoint."""
    return TextureEncoder(emb_size, hidden_dim, z_dim, num_channel, device).load_state_dict(_strip(state, "rhy_encoder"))


def split_pnotree_vae_state(state: Mapping[str, object]):
    """The key routing of utils.py:23-42: encoder parts to the encoder, everything else to the decoder, ``note_embedding.*`` to both."""
    enc_parts = ("note_embedding", "enc_notes_gru", "enc_time_gru", "linear_mu", "linear_std")
    enc_state, dec_state = {}, {}
    for k, v in state.items():
        part = k.split(".")[0]
        if part in enc_parts:
            enc_state[k] = v
            if part == "note_embedding":
                dec_state[k] = v
        else:
            dec_state[k] = v
    return enc_state, dec_state


def load_pretrained_pnotree_enc_dec(state, max_simu_note, device=None):
    """utils.py:19-45: a PianoTree VAE checkpoint (bare keys) -> (encoder, decoder); ``note_embedding.*`` goes to both."""
    if isinstance(state, (str, bytes)) or hasattr(state, "__fspath__"):
        from .checkpoint import load_legacy_pt
        state = load_legacy_pt(str(state))
    enc_state, dec_state = split_pnotree_vae_state(state)
    enc = PianoTreeEncoder(max_simu_note=max_simu_note, device=device)
    dec = PianoTreeDecoder(max_simu_note=max_simu_note, device=device)
    return enc.load_state_dict(enc_state), dec.load_state_dict(dec_state)


def load_pretrained_chd_enc_dec(state, input_dim, z_input_dim, hidden_dim, z_dim, n_step, device=None):
    """utils.py:48-69: the ``chord_enc.`` / ``chord_dec.`` keys of a chd_8bar checkpoint -> (encoder, decoder)."""
    enc = ChordEncoder(input_dim, hidden_dim, z_dim, device).load_state_dict(_strip(state, "chord_enc"))
    dec = ChordDecoder(input_dim, z_input_dim, hidden_dim, z_dim, n_step, device).load_state_dict(_strip(state, "chord_dec"))
    return enc, dec


class Polyffusion_SDF:
    def __init__(self, ldm: LatentDiffusion, cond_type, cond_mode="cond", chord_enc: Optional[ChordEncoder] = None,
                 chord_dec=None, pnotree_enc=None, pnotree_dec=None, txt_enc: Optional[TextureEncoder] = None,
                 concat_blurry=False, concat_ratio=1 / 8):
        self.ldm, self.cond_type, self.cond_mode = ldm, cond_type, cond_mode
        self.chord_enc, self.txt_enc, self.pnotree_enc = chord_enc, txt_enc, pnotree_enc
        self.chord_dec, self.pnotree_dec = chord_dec, pnotree_dec
        self.concat_blurry, self.concat_ratio = concat_blurry, concat_ratio

    @classmethod
    def load_trained(cls, ldm, chkpt_fpath, cond_type, cond_mode="cond", chord_enc=None, chord_dec=None,
                     pnotree_enc=None, pnotree_dec=None, txt_enc=None):
        """Legacy ``.pt`` (``{"model": state_dict}``, models/model_sdf.py:59-84) or Lightning ``.ckpt``
        (``model.``-prefixed ``state_dict``, inference_sdf.py:717-732) with ``ldm.eps_model.*``, ``chord_enc.*``,
        ``txt_enc.*`` keys and recomputable schedule vectors ``ldm.{alpha,beta,alpha_bar,sigma2}``."""
        from .checkpoint import load_checkpoint
        model = cls(ldm, cond_type, cond_mode, chord_enc, chord_dec, pnotree_enc, pnotree_dec, txt_enc)
        model.load_state_dict(load_checkpoint(chkpt_fpath)[0])
        return model

    def load_state_dict(self, state: Mapping[str, object]):
        from .checkpoint import split_state, split_state_decoders, split_state_full
        unet, ce, te = split_state(state)
        self.ldm.eps_model.load_state_dict(unet)
        dec = split_state_decoders(state)     # decoder keys go to an attached decoder; without one they are dropped
        if self.pnotree_dec is not None and dec["pnotree_dec"]:
            self.pnotree_dec.load_state_dict(dec["pnotree_dec"])
        if self.chord_dec is not None and dec["chord_dec"]:
            self.chord_dec.load_state_dict(dec["chord_dec"])
        pe = split_state_full(state)["pnotree_enc"]
        if self.pnotree_enc is not None and pe:
            self.pnotree_enc.load_state_dict(pe)
        if self.chord_enc is not None and ce:
            self.chord_enc.load_state_dict(ce)
        if self.txt_enc is not None and te:
            self.txt_enc.load_state_dict(te)
        return self

    def eval(self):
        return self

    def _encode_chord(self, chord: torch.Tensor) -> torch.Tensor:
        if self.chord_enc is not None:
            return self.chord_enc(chord).mean.unsqueeze(1)  # [B,1,512]
        return torch.reshape(chord, (-1, 1, chord.shape[1] * chord.shape[2]))

    def _decode_chord(self, z: torch.Tensor) -> torch.Tensor:
        """models/model_sdf.py:108-136: ``z`` [B, z_dim] -> [B, n_step, 36] int64 (one-hot root | chroma bits | one-hot bass); ``z``
        itself without a decoder."""
        if self.chord_dec is None:
            return z
        root, chroma, bass = self.chord_dec(z, inference=True, tfr=0.0)
        one_hot = torch.nn.functional.one_hot
        return torch.cat([one_hot(root.max(-1)[1], 12), chroma.max(-1)[1], one_hot(bass.max(-1)[1], 12)], dim=-1)

    def _decode_pnotree(self, z: torch.Tensor) -> torch.Tensor:
        """models/model_sdf.py:166-183: ``z`` [B, 1, 4*z_dim] (or [B, 4*z_dim]) -> the index grid [B, 128, S-1, 6] int64, the four
        two-bar segments of a sample along dim 1.  The four slices of every sample are decoded as ONE batch of 4B rows.
        Not kept from the reference: its ``z_seg.squeeze()`` also removes the batch dimension at B = 1 (and then fails inside the
        decoder); here B = 1 is one sample."""
        assert self.pnotree_dec is not None
        B = z.shape[0]
        rows = z.reshape(B * 4, -1)                            # rows (b, segment): [B, 4*z_dim] -> [4B, z_dim] is a pure view
        est = self.pnotree_dec.decode(rows)[2]                 # [4B, 32, S-1, 6]
        return est.view(B, 4 * 32, est.shape[2], 6)

    def _encode_pnotree(self, pnotree: torch.Tensor) -> torch.Tensor:
        """models/model_sdf.py:138-151: the four 2-bar segments of every sample through the encoder, means concatenated: [B,1,4z]."""
        assert self.pnotree_enc is not None
        B, S = pnotree.shape[0], pnotree.shape[2]
        segs = pnotree.contiguous().view(B * 4, 32, S, 6)      # [B,128,S,6] -> [B*4,32,S,6]: a pure view, rows (b, segment)
        return self.pnotree_enc(segs)[0].mean.view(B, 1, -1)

    def _encode_txt(self, prmat: torch.Tensor) -> torch.Tensor:
        if self.txt_enc is None:
            return prmat
        B = prmat.shape[0]
        # the four 2-bar segments of every sample go through the encoder as ONE batch of 4B rows;
        # [B,128,128] -> [B*4,32,128] is a pure view and the means come back as [B, 4*z] = cat(dim=-1)
        segs = prmat.contiguous().view(B * 4, 32, prmat.shape[2])
        return self.txt_enc(segs).mean.view(B, 1, -1)

    def get_loss_dict(self, batch, step, *, detail: bool = False, **loss_kw):
        """models/model_sdf.py:185-234: the condition of a reference-layout batch ``(prmat2c, pnotree, chord, prmat)`` by ``cond_type``
        (``chord`` | ``pnotree`` | ``txt`` | ``chord+txt``), replaced by all -1 under ``cond_mode`` ``uncond`` and, under ``mix`` /
        ``mix2``, with probability 0.2 - Python's ``random.random() < 0.2`` in the reference's call order (``chord+txt`` with ``mix2``:
        the chord draw, the texture draw, then the whole-condition draw), so a seeded ``random`` makes the reference's choices.  Returns
        ``{"loss": ldm.loss(prmat2c, cond)}``.

        ``concat_blurry``: at HEAD the reference calls ``exit(0)`` on this branch (:227-230); here it computes what the line after
        that says, ``ldm.loss(prmat2c, cond, cond_concat=get_blurry_image(prmat2c, ratio=concat_ratio))``.

        ``loss_kw`` (``noise``, ``t``, ``seed``, ``draw``, ``elem_offset``) go to ``ldm.loss``; ``detail=True`` adds the per-sample
        ``"loss_rows"`` (float64 ``[B]``) and the ``"t"`` they were evaluated at."""
        prmat2c, pnotree, chord, prmat = batch
        if self.cond_type == "chord":
            cond = self._encode_chord(chord)
        elif self.cond_type == "pnotree":
            cond = self._encode_pnotree(pnotree)
        elif self.cond_type == "txt":
            cond = self._encode_txt(prmat)
        elif self.cond_type == "chord+txt":
            zchd = self._encode_chord(chord)
            ztxt = self._encode_txt(prmat)
            if self.cond_mode == "mix2":
                if random.random() < 0.2:
                    zchd = -torch.ones_like(zchd)
                if random.random() < 0.2:
                    ztxt = -torch.ones_like(ztxt)
            cond = torch.cat([zchd, ztxt], dim=-1)
        else:
            raise NotImplementedError(f"cond_type {self.cond_type!r}")
        if self.cond_mode == "uncond":
            cond = -torch.ones_like(cond)
        elif self.cond_mode in ("mix", "mix2"):
            if random.random() < 0.2:
                cond = -torch.ones_like(cond)
        cond_concat = None
        if self.concat_blurry:
            from .inference_sdf import get_blurry_image
            cond_concat = get_blurry_image(prmat2c, ratio=self.concat_ratio)
        if not detail:
            return {"loss": self.ldm.loss(prmat2c, cond, cond_concat=cond_concat, **loss_kw)}
        rows, t = self.ldm.loss_rows(prmat2c, cond, cond_concat=cond_concat, return_t=True, **loss_kw)
        return {"loss": rows.mean().float(), "loss_rows": rows, "t": t}
