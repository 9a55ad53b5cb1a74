"""Polydis inference on the HIP path: ``DisentangleVAE`` (``polydis/model.py``), its ``PtvaeDecoder`` (``polydis/ptvae.py``) and
``PolydisAftertouch`` (``polydis_aftertouch.py``) of the reference.

* ``PtvaeDecoder`` is ``decoders.PianoTreeDecoder`` with the defaults of ``polydis/ptvae.py`` (``max_simu_note=32``); the two reference
  classes are the same statements.  ``DisentangleVAE.init_model`` builds it with ``dec_dur_hid_size=64``.
* The two encoders are the ``pf_encoder`` handles of ``model_sdf`` created with the scale head (``pf_encoder_forward_dist``): the
  Normal's ``mean`` and ``scale = exp(linear_var(h))``.
* ``chd_decoder.*`` (``ptvae.RnnDecoder``) is accepted and checked against ``arch`` but no inference method runs it: no handle is built.

``z`` stays on the device between the encoders and the decoder; the only host copy is the final integer grid.  Training entry points
(``run``, ``loss*``, ``confuse_prmat``) raise ``NotImplementedError``.

Random draws (``sample=True``, ``chd_sample``, ``posterior_sample``, ``prior_sample``) are ``mean + scale * torch.randn(...,
generator=generator)`` on the device.  They follow the reference's distributions but are NOT bit-comparable with its draws, which
come from torch's global generator through ``Normal.rsample`` / ``.sample`` on whatever device the reference model sits on.
"""
from __future__ import annotations

import os
from types import SimpleNamespace
from typing import Mapping, Optional

import numpy as np
import torch

from . import _lib, midi
from .arch import chord_decoder_param_shapes
from .decoders import PianoTreeDecoder
from .model_sdf import ChordEncoder, TextureEncoder

MODEL_PATH = "pretrained/polydis/model_master_final.pt"     # polydis_aftertouch.py:6


class PtvaeDecoder(PianoTreeDecoder):
    """``polydis/ptvae.py:PtvaeDecoder``: ``PianoTreeDecoder`` with ``max_simu_note=32``."""

    def __init__(self, note_embedding=None, max_simu_note=32, dec_dur_hid_size=16, **kw):
        super().__init__(note_embedding=note_embedding, max_simu_note=max_simu_note, dec_dur_hid_size=dec_dur_hid_size, **kw)

    def output_to_numpy(self, recon_pitch, recon_dur):
        """``ptvae.py`` ``output_to_numpy``: ``(est_x [R,32,S-1,6] int64, est_pitch, est_dur)`` as numpy arrays."""
        est_pitch = recon_pitch.max(-1)[1].unsqueeze(-1)
        est_dur = recon_dur.max(-1)[1]
        est_x = torch.cat([est_pitch, est_dur], dim=-1)
        return est_x.cpu().numpy(), est_pitch.cpu().numpy(), est_dur.cpu().numpy()


def _randn(like: torch.Tensor, generator) -> torch.Tensor:
    dev = generator.device if generator is not None else like.device
    return torch.randn(like.shape, generator=generator, device=dev, dtype=torch.float32).to(like.device)


def _draw(dist, generator) -> torch.Tensor:
    return dist.mean + dist.scale * _randn(dist.mean, generator)


class DisentangleVAE:
    PARTS = ("chd_encoder", "rhy_encoder", "decoder", "chd_decoder")

    def __init__(self, name, chd_encoder: ChordEncoder, rhy_encoder: TextureEncoder, decoder: PtvaeDecoder, chd_decoder_shapes):
        self.name = name
        self.chd_encoder, self.rhy_encoder, self.decoder = chd_encoder, rhy_encoder, decoder
        self.chd_decoder_shapes = chd_decoder_shapes          # ptvae.RnnDecoder: keys and shapes only
        self.num_step = decoder.num_step

    @staticmethod
    def init_model(chd_size=256, txt_size=256, num_channel=10, device=None) -> "DisentangleVAE":
        """polydis/model.py:303-319."""
        if chd_size + txt_size != 512:
            raise ValueError("DisentangleVAE: the decoder is built for z_size = chd_size + txt_size = 512")
        chd_encoder = ChordEncoder(36, 1024, chd_size, device, with_scale=True)
        rhy_encoder = TextureEncoder(256, 1024, txt_size, num_channel, device, with_scale=True)
        decoder = PtvaeDecoder(note_embedding=None, dec_dur_hid_size=64, z_size=chd_size + txt_size, device=device)
        return DisentangleVAE("disvae", chd_encoder, rhy_encoder, decoder, chord_decoder_param_shapes(36, 256, 512, chd_size))

    # ---------------------------------------------------------------------------------------------- weights
    def split_state_dict(self, state: Mapping[str, object]):
        """``module.`` stripped, keys routed by their first component; anything else is an unexpected key."""
        parts = {p: {} for p in self.PARTS}
        for k, v in state.items():
            k = k.replace("module.", "")                      # model.py:323-324
            head, _, rest = k.partition(".")
            if head not in parts or not rest:
                raise RuntimeError(f"load_state_dict({k}): unexpected key '{k}' (not a parameter of this DisentangleVAE)")
            parts[head][rest] = v
        return parts

    def _check_chd_decoder(self, state: Mapping[str, object]):
        for k, v in state.items():
            if k not in self.chd_decoder_shapes:
                raise RuntimeError(f"chd_decoder: load_state_dict({k}): unexpected key '{k}' (not a parameter of this decoder)")
            got, want = tuple(np.shape(v)), tuple(self.chd_decoder_shapes[k])
            if got != want:
                fmt = lambda s: "".join(f"{d}," for d in s)
                raise RuntimeError(f"chd_decoder: load_state_dict({k}): size mismatch for '{k}': expected [{fmt(want)}] got [{fmt(got)}]")
        missing = [k for k in self.chd_decoder_shapes if k not in state]
        if missing:
            raise RuntimeError(f"chd_decoder: load_state_dict: {len(missing)} missing key(s), first: {missing[0]}")

    def pack_state_dict(self, state: Mapping[str, object]):
        """Host half of ``load_state_dict`` (no GPU needed): the three packed blobs, every message of the load included - the
        handles' own wording (missing / unexpected key, size mismatch) behind the name of the part it concerns."""
        parts = self.split_state_dict(state)
        self._check_chd_decoder(parts["chd_decoder"])
        blobs = {}
        for p in ("chd_encoder", "rhy_encoder", "decoder"):
            try:
                blobs[p] = getattr(self, p).pack_state_dict(parts[p])
            except RuntimeError as e:
                raise RuntimeError(f"{p}: {e}") from None
        return blobs

    def load_state_dict(self, state: Mapping[str, object]):
        """Route ``chd_encoder.*`` / ``rhy_encoder.*`` / ``decoder.*`` to their handles (pack on the host, copy, bind); ``chd_decoder.*`` is
        checked against ``arch`` and dropped."""
        blobs = self.pack_state_dict(state)
        _lib.require_gpu()
        for p, blob in blobs.items():
            mod = getattr(self, p)
            mod.bind_packed(blob.to(mod.device))
        return self

    def load_model(self, model_path: str):
        """model.py:321-325, through the restricted loader of ``checkpoint.py``."""
        from .checkpoint import load_legacy_pt
        return self.load_state_dict(load_legacy_pt(model_path))

    def eval(self):
        return self

    # ---------------------------------------------------------------------------------------------- inference
    def _dev(self):
        return self.decoder.device

    def inference_encode(self, pr_mat, c):
        """-> ``(dist_chd, dist_rhy)``: objects with ``.mean`` and ``.scale`` [R, 256] on the device."""
        dev = self._dev()
        c = torch.as_tensor(c).to(dev, torch.float32)
        pr_mat = torch.as_tensor(pr_mat).to(dev, torch.float32)
        m_c, s_c = self.chd_encoder.encode_dist(c)
        m_r, s_r = self.rhy_encoder.encode_dist(pr_mat)
        return SimpleNamespace(mean=m_c, scale=s_c), SimpleNamespace(mean=m_r, scale=s_r)

    def inference_decode(self, z_chd, z_rhy) -> np.ndarray:
        """-> ``est_x`` [R, 32, 31, 6] int64 numpy (``output_to_numpy``)."""
        dev = self._dev()
        dec_z = torch.cat([torch.as_tensor(z_chd).to(dev, torch.float32), torch.as_tensor(z_rhy).to(dev, torch.float32)], dim=-1)
        return self.decoder.decode(dec_z)[2].cpu().numpy()

    def inference(self, pr_mat, c, sample, chd_sample=False, generator=None) -> np.ndarray:
        """model.py:188-200.  Draw order with a generator: z_chd, z_rhy (``sample``), then the N(0, 1) z_chd of ``chd_sample``."""
        dist_chd, dist_rhy = self.inference_encode(pr_mat, c)
        z_chd, z_rhy = (_draw(dist_chd, generator), _draw(dist_rhy, generator)) if sample else (dist_chd.mean, dist_rhy.mean)
        if chd_sample:
            z_chd = _randn(z_chd, generator)
        return self.inference_decode(z_chd, z_rhy)

    def swap(self, pr_mat1, pr_mat2, c1, c2, fix_rhy, fix_chd) -> np.ndarray:
        return self.inference(pr_mat1 if fix_rhy else pr_mat2, c1 if fix_chd else c2, sample=False)

    def posterior_sample(self, pr_mat, c, scale=None, sample_chd=True, sample_txt=True, generator=None) -> np.ndarray:
        """model.py:208-228.  Both latents are drawn (z_chd first) and the one not asked for is replaced by its mean, as there."""
        if scale is None and sample_chd and sample_txt:
            return self.inference(pr_mat, c, sample=True, generator=generator)
        dist_chd, dist_rhy = self.inference_encode(pr_mat, c)
        if scale is not None:
            dist_chd = SimpleNamespace(mean=dist_chd.mean, scale=dist_chd.scale * scale)
            dist_rhy = SimpleNamespace(mean=dist_rhy.mean, scale=dist_rhy.scale * scale)
        z_chd, z_rhy = _draw(dist_chd, generator), _draw(dist_rhy, generator)
        if not sample_chd:
            z_chd = dist_chd.mean
        if not sample_txt:
            z_rhy = dist_rhy.mean
        return self.inference_decode(z_chd, z_rhy)

    def prior_sample(self, x, c, sample_chd=False, sample_rhy=False, scale=1.0, generator=None) -> np.ndarray:
        """model.py:230-239: N(0, scale) in place of a posterior; the posterior that stays is still sampled, as there."""
        dist_chd, dist_rhy = self.inference_encode(x, c)
        prior = SimpleNamespace(mean=torch.zeros_like(dist_rhy.mean), scale=torch.ones_like(dist_rhy.mean) * scale)
        if sample_chd:
            dist_chd = prior
        if sample_rhy:
            dist_rhy = prior
        return self.inference_decode(_draw(dist_chd, generator), _draw(dist_rhy, generator))

    def gt_sample(self, x):
        return (x.cpu() if isinstance(x, torch.Tensor) else torch.as_tensor(x))[:, :, 1:].numpy()

    def interp(self, pr_mat1, c1, pr_mat2, c2, interp_chd=False, interp_rhy=False, int_count=10) -> np.ndarray:
        """model.py:245-265; the paths are host numpy, as in the reference.  -> [bs, int_count, 32, 31, 6]
        (the reference reshapes to 15 slots, which fits only a 16-note decoder)."""
        dist_chd1, dist_rhy1 = self.inference_encode(pr_mat1, c1)
        dist_chd2, dist_rhy2 = self.inference_encode(pr_mat2, c2)
        z_chd1, z_rhy1, z_chd2, z_rhy2 = (d.mean.cpu() for d in (dist_chd1, dist_rhy1, dist_chd2, dist_rhy2))
        z_chds = self.interp_z(z_chd1, z_chd2, int_count) if interp_chd else z_chd1.unsqueeze(1).repeat(1, int_count, 1)
        z_rhys = self.interp_z(z_rhy1, z_rhy2, int_count) if interp_rhy else z_rhy1.unsqueeze(1).repeat(1, int_count, 1)
        bs = z_chds.size(0)
        estxs = self.inference_decode(z_chds.reshape(bs * int_count, -1), z_rhys.reshape(bs * int_count, -1))
        return estxs.reshape((bs, int_count, 32, self.decoder.max_simu_note - 1, -1))

    def interp_z(self, z1, z2, int_count=10) -> torch.Tensor:
        z1, z2 = (z.cpu().numpy() if isinstance(z, torch.Tensor) else np.asarray(z) for z in (z1, z2))
        return torch.stack([self.interp_path(a, b, int_count) for a, b in zip(z1, z2)], dim=0)

    def interp_path(self, z1, z2, interpolation_count=10) -> torch.Tensor:
        """model.py:275-300: spherical interpolation of the directions, log-linear interpolation of the norms."""
        result_shape = z1.shape
        z1, z2 = z1.reshape(-1), z2.reshape(-1)

        def slerp2(p0, p1, t):
            omega = np.arccos(np.dot(p0 / np.linalg.norm(p0), p1 / np.linalg.norm(p1)))
            so = np.sin(omega)
            return np.sin((1.0 - t) * omega)[:, None] / so * p0[None] + np.sin(t * omega)[:, None] / so * p1[None]

        percentages = np.linspace(0.0, 1.0, interpolation_count)
        dirs = slerp2(z1 / np.linalg.norm(z1), z2 / np.linalg.norm(z2), percentages)
        length = np.linspace(np.log(np.linalg.norm(z1)), np.log(np.linalg.norm(z2)), interpolation_count)
        out = (dirs * np.exp(length[:, None])).reshape([interpolation_count] + list(result_shape))
        return torch.from_numpy(out).float()

    # ---------------------------------------------------------------------------------------------- training: not on this path
    def _training(self, *a, **k):
        raise NotImplementedError("DisentangleVAE: training code (run, loss, confuse_prmat) is not implemented; inference only")

    run = loss = loss_function = chord_loss = kl_loss = confuse_prmat = _training


class PolydisAftertouch:
    """``polydis_aftertouch.py:19-30``.  ``state``: a state_dict to load instead of ``model_path`` (e.g. ``weights.synth_polydis_state``)."""

    def __init__(self, model_path: str = MODEL_PATH, state: Optional[Mapping[str, object]] = None, device=None, say=print):
        model = DisentangleVAE.init_model(device=device)
        if state is not None:
            model.load_state_dict(state)
        else:
            if not os.path.exists(model_path):
                raise RuntimeError(f"{model_path}: no Polydis checkpoint there (give a path, or a state_dict)")
            model.load_model(model_path)
            say(f"loaded model {model_path}.")
        self.model = model

    def reconstruct(self, prmat, chd, fn, chd_sample=False, generator=None) -> np.ndarray:
        """``prmat`` [R,32,128], ``chd`` [R,8,36] -> the decoded grid, written to ``fn`` (``estx_to_midi_file``) and returned."""
        est_x = self.model.inference(torch.as_tensor(prmat).float(), torch.as_tensor(chd).float(), sample=False, chd_sample=chd_sample,
                                     generator=generator)
        midi.estx_to_midi_file(est_x, fn)
        return est_x
