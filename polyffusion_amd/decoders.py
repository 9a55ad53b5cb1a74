"""Frozen decoders of ``Polyffusion_SDF`` in inference mode, on the ``pf_decoder`` handle of libpfhip.so.

* ``PianoTreeDecoder``: ``dl_modules/pianotree_dec.py:10-99`` (constructor keywords and order kept), ``forward`` = ``:334-339``.
* ``ChordDecoder``: ``dl_modules/chord_dec.py:7-25``, ``forward`` = ``:27-70``.

Both are greedy decodes: every arg-max is fed back as the next token, on the device.  Teacher forcing exists for the chord decoder
only, as ``ChordDecoder.forward_forced`` (``chord_dec.py:27-70`` with ``inference=False``; forward pass, for the chd_8bar objective).
No torch module takes part; without the library / a GPU ``forward`` raises.
"""
from __future__ import annotations

import ctypes as C
from typing import Sequence, Union

import torch

from . import _lib
from ._handle import ModelHandle


class _Decoder(ModelHandle):
    PREFIX = "pf_decoder"

    def n_launches(self, rows: int = 1) -> int:
        """Kernel launches of one decode (a dry run of the plan: no GPU needed)."""
        return int(self._lib.pf_decoder_launches(self._h, rows))

    def _z(self, z: torch.Tensor, width: int) -> torch.Tensor:
        if self._blob_dev is None:
            raise RuntimeError("decoder weights not loaded")
        if z.dim() != 2 or z.shape[1] != width or z.shape[0] < 1:
            raise RuntimeError(f"decoder input must be [rows, {width}], got {tuple(z.shape)}")
        return z.detach().to(device=self.device, dtype=torch.float32).contiguous()

    def _forward(self, z, out0, out1, out2, est):
        ws = self.workspace_for(self._lib.pf_decoder_workspace_bytes(self._h, z.shape[0]), z.device)
        self._check(self._lib.pf_decoder_forward(self._h, z.data_ptr(), z.shape[0], out0.data_ptr(), out1.data_ptr(), _lib.ptr(out2),
                                                 _lib.ptr(est), ws.data_ptr(), ws.numel(), _lib.current_stream()), "pf_decoder_forward")


class PianoTreeDecoder(_Decoder):
    """``PianoTreeDecoder(...)`` of the reference at its default sizes; ``max_simu_note`` (at most 32) is free, and ``dec_dur_hid_size``
    is 16 (the default) or 64 (what Polydis builds, ``polydis/model.py:314-316``)."""
    KIND = 1

    def __init__(self, note_embedding=None, max_simu_note=20, max_pitch=127, min_pitch=0, pitch_sos=128, pitch_eos=129, pitch_pad=130,
                 dur_pad=2, dur_width=5, num_step=32, note_emb_size=128, z_size=512, dec_emb_hid_size=128, dec_time_hid_size=1024,
                 dec_notes_hid_size=512, dec_z_in_size=256, dec_dur_hid_size=16, device=None):
        if note_embedding is not None:
            raise ValueError("PianoTreeDecoder: a shared note_embedding module is not supported; its tensors arrive as note_embedding.* keys")
        got = (max_pitch, min_pitch, pitch_sos, pitch_eos, pitch_pad, dur_pad, dur_width, num_step, note_emb_size, z_size, dec_emb_hid_size,
               dec_time_hid_size, dec_notes_hid_size, dec_z_in_size)
        if got != (127, 0, 128, 129, 130, 2, 5, 32, 128, 512, 128, 1024, 512, 256):
            raise ValueError("PianoTreeDecoder: only the reference's default sizes are built (max_simu_note is free)")
        if dec_dur_hid_size not in (16, 64):
            raise ValueError(f"PianoTreeDecoder: dec_dur_hid_size must be 16 or 64, got {dec_dur_hid_size}")
        if not 2 <= max_simu_note <= 32:
            raise ValueError("PianoTreeDecoder: max_simu_note must be in 2..32")
        self.max_simu_note, self.num_step, self.z_size = max_simu_note, num_step, z_size
        self.pitch_range, self.dur_width, self.dec_dur_hid_size = 130, dur_width, dec_dur_hid_size
        super().__init__(_lib.load(), self.KIND, max_simu_note, 0, 0, dec_dur_hid_size, 0, 0, device=device)   # hidden_dim = the duration width

    def decode(self, z: torch.Tensor):
        """``z`` [R, 512] -> ``(recon_pitch [R,32,S-1,130], recon_dur [R,32,S-1,5,2], est [R,32,S-1,6] int64)``; ``est`` is the
        ``max(-1)[1]`` of the two logit tensors (pitch index, five duration digits), taken on the device (ties: lowest index)."""
        z = self._z(z, self.z_size)
        R, n = z.shape[0], self.max_simu_note - 1
        pitch = torch.empty(R, 32, n, 130, dtype=torch.float32, device=z.device)
        dur = torch.empty(R, 32, n, 5, 2, dtype=torch.float32, device=z.device)
        est = torch.empty(R, 32, n, 6, dtype=torch.int32, device=z.device)
        self._forward(z, pitch, dur, None, est)
        return pitch, dur, est.long()

    def forward(self, z, inference, x, lengths, teacher_forcing_ratio1, teacher_forcing_ratio2):
        if not inference:
            raise NotImplementedError("PianoTreeDecoder: teacher forcing (training) is not implemented; inference=True only")
        assert x is None and lengths is None and teacher_forcing_ratio1 == 0 and teacher_forcing_ratio2 == 0
        return self.decode(z)[:2]

    __call__ = forward


class ChordDecoder(_Decoder):
    KIND = 0

    def __init__(self, input_dim=36, z_input_dim=256, hidden_dim=512, z_dim=256, n_step=8, device=None):
        self.input_dim, self.hidden_dim, self.z_dim, self.n_step = input_dim, hidden_dim, z_dim, n_step
        super().__init__(_lib.load(), self.KIND, 0, input_dim, z_input_dim, hidden_dim, z_dim, n_step, device=device)

    def forward(self, z_chd, inference, tfr, gt_chd=None):
        """``z_chd`` [R, z_dim] -> ``(recon_root [R,n_step,12], recon_chroma [R,n_step,12,2], recon_bass [R,n_step,12])``."""
        if not inference:
            raise NotImplementedError("ChordDecoder.forward: teacher forcing (training) is not implemented here, inference=True only; "
                                      "ChordDecoder.forward_forced runs the teacher-forced decode")
        z = self._z(z_chd, self.z_dim)
        R = z.shape[0]
        root = torch.empty(R, self.n_step, 12, dtype=torch.float32, device=z.device)
        chroma = torch.empty(R, self.n_step, 12, 2, dtype=torch.float32, device=z.device)
        bass = torch.empty(R, self.n_step, 12, dtype=torch.float32, device=z.device)
        self._forward(z, root, chroma, bass, None)
        return root, chroma, bass

    __call__ = forward

    def force_mask(self, force: Union[int, Sequence[bool]]) -> int:
        """``force`` as the library's bit mask: a sequence of ``n_step - 1`` booleans (entry ``t``: feed ``gt[:, t]`` to step ``t + 1``)
        or an int whose bit ``t`` says the same."""
        n = self.n_step - 1
        if isinstance(force, int) and not isinstance(force, bool):
            if force < 0 or force >> max(n, 0):
                raise ValueError(f"ChordDecoder: force mask {force:#x} has bits past step {n - 1}")
            return force
        flips = [bool(f) for f in force]
        if len(flips) != n:
            raise ValueError(f"ChordDecoder: force needs n_step - 1 = {n} entries, got {len(flips)}")
        return sum(1 << t for t, f in enumerate(flips) if f)

    def n_launches_forced(self, rows: int = 1, feedback: str = "row") -> int:
        """The most launches one ``forward_forced`` enqueues (mask 0; a dry run, no GPU needed)."""
        return int(self._lib.pf_decoder_forced_launches(self._h, rows, _lib.FEEDBACK[feedback]))

    def forward_forced(self, z_chd, gt_chd, force: Union[int, Sequence[bool]] = 0, feedback: str = "row"):
        """``ChordDecoder.forward(z_chd, False, tfr, gt_chd)`` of the reference with its coin flips handed in: where ``force[t]`` is set
        the token fed to step ``t + 1`` is ``gt_chd[:, t]``, elsewhere the arg-max token of step ``t``.  ``feedback="row"``: each row
        feeds back its own arg-max (batch-invariant; mask 0 is ``forward(z, True, 0)`` bit for bit).  ``feedback="batch"``: the
        reference's token at batch > 1, whose root / bass part is the union over the rows of THIS call (``chord_dec.py:59-63``).
        Returns ``(recon_root [R,n_step,12], recon_chroma [R,n_step,12,2], recon_bass [R,n_step,12])``."""
        if feedback not in _lib.FEEDBACK:
            raise ValueError(f"ChordDecoder: feedback must be 'row' or 'batch', got {feedback!r}")
        mask = self.force_mask(force)
        z = self._z(z_chd, self.z_dim)
        R = z.shape[0]
        if tuple(gt_chd.shape) != (R, self.n_step, 36):
            raise RuntimeError(f"ChordDecoder: gt_chd must be [{R}, {self.n_step}, 36], got {tuple(gt_chd.shape)}")
        gt = gt_chd.detach().to(device=z.device, dtype=torch.float32).contiguous()
        root = torch.empty(R, self.n_step, 12, dtype=torch.float32, device=z.device)
        chroma = torch.empty(R, self.n_step, 12, 2, dtype=torch.float32, device=z.device)
        bass = torch.empty(R, self.n_step, 12, dtype=torch.float32, device=z.device)
        ws = self.workspace_for(self._lib.pf_decoder_forced_workspace_bytes(self._h, R), z.device)
        a = _lib.ChordForcedArgs(z=z.data_ptr(), gt=gt.data_ptr(), rows=R, feedback=_lib.FEEDBACK[feedback], force_mask=mask,
                                 root=root.data_ptr(), chroma=chroma.data_ptr(), bass=bass.data_ptr(), workspace=ws.data_ptr(),
                                 workspace_bytes=ws.numel())
        self._check(self._lib.pf_decoder_forward_forced(self._h, C.byref(a), _lib.current_stream()), "pf_decoder_forward_forced")
        return root, chroma, bass
