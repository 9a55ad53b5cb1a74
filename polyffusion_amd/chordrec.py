"""Recognise the chords of generated rolls on the GPU (an extension built on the reference's own rule-based extractor).

``recognize_rolls`` is one HIP launch (``pf_chord_recognize``, include/pfhip.h) over the images where the sampler left them.  Per song of
``segments`` consecutive images it gives, beat by beat, the label ``chord_extractor.recognize`` returns for the file
``midi.prmat2c_to_midi_file`` would write - the template matching plus dynamic programme that produces every chord condition of the
``--from_midi`` path - and the condition row that label stands for, and compares those rows with the chords the run was conditioned on:
do the chords the model was given come back out of what it generated, by the rule that made them?

Two deviations from the file path: a song always has ``segments * steps / 4`` beats (the file path counts beats up to the last note-off),
and a song without notes is all ``N`` (the file path fails on it).  The 529 labels of the vocabulary stand for 325 distinct rows (a 9th,
11th or 13th chord is encoded as its seventh chord), so ``chord_acc`` compares rows, not names.  The ``N`` row has bits 34 and 35 set: the
``root = -1`` indexing of ``chd_to_onehot(chord_matrix_from_labels(...))``, kept because that is what ``--from_midi`` conditions on.

``chord_acc = FULL_HIT / BEATS``: the share of beats whose root, chroma bits and bass all agree; ``root_acc``, ``chroma_acc``, ``bass_acc``
the three on their own; ``chroma_iou = CHROMA_INTER / CHROMA_UNION`` over the song.  0 / 0 is 0.0.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import Dict, List, Optional

import numpy as np
import torch

from . import _lib

IDX = {n: i for i, n in enumerate(_lib.CHORDREC_COUNTERS)}
SCORES = ("chord_acc", "root_acc", "chroma_acc", "bass_acc", "chroma_iou")
_HITS = {"chord_acc": "FULL_HIT", "root_acc": "ROOT_HIT", "chroma_acc": "CHROMA_HIT", "bass_acc": "BASS_HIT"}

_HOST = None
_DEVICE: Dict[tuple, tuple] = {}


def vocabulary_tables() -> dict:
    """The vocabulary as the host arrays ``pf_chord_recognize`` reads (built once): ``names`` (529 labels of ``ChordClass``), ``cls_bits``
    int32 (template | bass class << 12 | size << 16), ``cls_const`` float64 ``[n, 2]`` (``size * 0.1`` and ``("/" in label) * 0.05`` as
    ``ChordClass.batch_score`` computes them), ``cls_rows`` float32 ``[n, 36]`` (``chd_to_onehot(chord_matrix_from_labels(...))``) and
    ``consts`` float64 ``[16]`` (``j * 0.7`` for j < 12, 0.15, 0.2, the 0.2 of ``N``, 0).  The constants travel as data so that the
    device adds the very bit patterns Python does."""
    global _HOST
    if _HOST is None:
        from .chord_extractor import ChordClass, chord_matrix_from_labels
        from .datasample import chd_to_onehot
        cc = ChordClass()
        n = len(cc.chord_list)
        bits, const = np.zeros(n, np.int32), np.zeros((n, 2), np.float64)
        for i, name in enumerate(cc.chord_list):
            tpl = cc.chroma_templates[i] > 0
            size = tpl.sum()
            bass = int(np.argmax(cc.bass_templates[i])) if size else 0
            bits[i] = sum(1 << k for k in range(12) if tpl[k]) | (bass << 12) | (int(size) << 16)
            const[i] = (size * 0.1, ("/" in name) * 0.05)
        rows = np.concatenate([chd_to_onehot(chord_matrix_from_labels([[0, .5, name]])) for name in cc.chord_list]).astype(np.float32)
        consts = np.array([j * 0.7 for j in range(12)] + [0.15, 0.2, 0.2, 0.0], np.float64)
        _HOST = dict(names=list(cc.chord_list), cls_bits=bits, cls_const=const, cls_rows=rows, consts=consts,
                     max_template=int(((bits >> 16) & 15).max()))
    return _HOST


def _device_tables(device: torch.device) -> tuple:
    key = (device.index if device.index is not None else torch.cuda.current_device(), _lib.X3_VARIANT)
    if key not in _DEVICE:
        t = vocabulary_tables()
        _DEVICE[key] = tuple(torch.from_numpy(t[k]).to(device).contiguous() for k in ("cls_bits", "cls_const", "cls_rows", "consts"))
    return _DEVICE[key]


def _ratio(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """a / b in float64 on int64 tensors, 0.0 where b == 0 (``score._ratio``)"""
    ok = b != 0
    return torch.where(ok, a.double() / torch.where(ok, b, torch.ones_like(b)).double(), torch.zeros((), dtype=torch.float64, device=a.device))


def scores_of(counters: torch.Tensor) -> Dict[str, torch.Tensor]:
    """The five ratios of ``counters [songs, 8]``: name -> float64 ``[songs]`` where the counters live."""
    g = lambda name: counters[:, IDX[name]].to(torch.int64)
    out = {k: _ratio(g(h), g("BEATS")) for k, h in _HITS.items()}
    out["chroma_iou"] = _ratio(g("CHROMA_INTER"), g("CHROMA_UNION"))
    return out


@dataclass
class ChordRecognition:
    """The device tensors of one ``pf_chord_recognize`` call: ``labels [songs, beats]`` int32 (index into ``vocabulary_tables()["names"]``),
    ``bounds [songs, beats]`` int32 (1 on the first beat of every recognised segment), ``rows [songs, beats, 36]`` float32 (the condition row
    of the label: what ``--from_midi`` would have produced), ``counters [songs, 8]`` int32 (``_lib.CHORDREC_COUNTERS``), ``path_score
    [songs]`` float64, ``chroma_q`` / ``bass_q [songs, beats, 12]`` int32 (quarter / eighth beats)."""
    labels: torch.Tensor
    bounds: torch.Tensor
    rows: torch.Tensor
    counters: torch.Tensor
    path_score: torch.Tensor
    chroma_q: torch.Tensor
    bass_q: torch.Tensor

    def counter(self, name: str) -> torch.Tensor:
        return self.counters[:, IDX[name]].to(torch.int64)

    def names(self) -> List[List[str]]:
        """Label strings per song and beat (one host copy)"""
        names = vocabulary_tables()["names"]
        return [[names[i] for i in song] for song in self.labels.tolist()]

    def lab_rows(self, song: int = 0) -> List[list]:
        """``[start, end, label]`` per recognised segment of one song, exactly as ``chord_extractor.transcribe_midi`` returns them for the
        written file: the song's images on one time axis, 0.5 s beats."""
        names = vocabulary_tables()["names"]
        labels, bounds = self.labels[song].tolist(), self.bounds[song].tolist()
        first = [i for i, b in enumerate(bounds) if b]
        return [[np.float64(a * 0.5), np.float64(b * 0.5), names[labels[a]]] for a, b in zip(first, first[1:] + [len(labels)])]

    def scores(self) -> Dict[str, torch.Tensor]:
        return scores_of(self.counters)

    def report(self) -> list:
        """Per song: the five scores as Python floats, the named counters as ints, the label names (one host copy each)."""
        sc = {k: v.tolist() for k, v in self.scores().items()}
        cnt, names = self.counters.tolist(), self.names()
        return [dict({k: sc[k][i] for k in SCORES}, counters={n: int(cnt[i][j]) for n, j in IDX.items()}, labels=names[i]) for i in range(len(cnt))]


def recognize_rolls(prmat2c: torch.Tensor, segments: int = 1, chord: Optional[torch.Tensor] = None, *, custom_round: bool = False,
                    bass_relative: bool = False) -> ChordRecognition:
    """``prmat2c [..., 2, steps, 128]`` (any leading shape, flattened to images; ``segments`` consecutive images are one song on one time
    axis) on the GPU -> ``ChordRecognition``, one launch on the current stream, no synchronisation.  ``chord``: ``songs * beats`` rows of 36
    in the songs' order, in any shape; without it the comparison counters are 0.  ``steps`` must be whole bars of 16 steps and a song at
    most ``_lib.CHORDREC_MAX_BEATS`` beats."""
    _lib.require_gpu()
    lib = _lib.load()
    if prmat2c.dim() < 4 or prmat2c.shape[-3] != 2 or prmat2c.shape[-1] != 128:
        raise ValueError(f"recognize_rolls: prmat2c must be [..., 2, steps, 128], got {tuple(prmat2c.shape)}")
    steps, segments = int(prmat2c.shape[-2]), int(segments)
    if steps <= 0 or steps % 16 != 0:
        raise ValueError(f"recognize_rolls: steps = {steps} is not a whole number of bars (16 steps each)")
    dev = prmat2c.device if prmat2c.is_cuda else torch.device("cuda", torch.cuda.current_device())
    x = prmat2c.detach().to(device=dev, dtype=torch.float32).reshape(-1, 2, steps, 128).contiguous()
    n = int(x.shape[0])
    if n == 0 or segments < 1 or n % segments != 0:
        raise ValueError(f"recognize_rolls: {n} images are not whole songs of {segments} segments")
    songs, beats = n // segments, segments * steps // 4
    if beats > _lib.CHORDREC_MAX_BEATS:
        raise ValueError(f"recognize_rolls: {segments} segments of {steps} steps are {beats} beats, more than {_lib.CHORDREC_MAX_BEATS} per song")
    if chord is not None:
        if chord.numel() != songs * beats * 36:
            raise ValueError(f"recognize_rolls: {songs} songs of {beats} beats need {songs * beats} chord rows of 36, got {tuple(chord.shape)}")
        chord = chord.detach().to(device=x.device, dtype=torch.float32).reshape(songs, beats, 36).contiguous()
    bits, const, rows, consts = _device_tables(x.device)
    host = vocabulary_tables()
    i32 = dict(dtype=torch.int32, device=x.device)
    out = ChordRecognition(torch.empty(songs, beats, **i32), torch.empty(songs, beats, **i32),
                           torch.empty(songs, beats, 36, dtype=torch.float32, device=x.device), torch.empty(songs, _lib.CHORDREC_NCOUNT, **i32),
                           torch.empty(songs, dtype=torch.float64, device=x.device), torch.empty(songs, beats, 12, **i32),
                           torch.empty(songs, beats, 12, **i32))
    a = _lib.ChordRecognizeArgs(prmat2c=x.data_ptr(), chord=_lib.ptr(chord) or None, cls_bits=bits.data_ptr(), cls_const=const.data_ptr(),
                                cls_rows=rows.data_ptr(), consts=consts.data_ptr(), songs=songs, segments=segments, steps=steps,
                                n_classes=len(host["names"]), max_template=host["max_template"], custom_round=int(bool(custom_round)),
                                bass_relative=int(bool(bass_relative)), reserved=0, labels=out.labels.data_ptr(), bounds=out.bounds.data_ptr(),
                                rows=out.rows.data_ptr(), counters=out.counters.data_ptr(), path_score=out.path_score.data_ptr(),
                                chroma_q=out.chroma_q.data_ptr(), bass_q=out.bass_q.data_ptr())
    _lib.check(lib.pf_chord_recognize(C.byref(a), _lib.current_stream()), "pf_chord_recognize", lib)
    return out


def write_lab(path: str, rows: List[list]) -> None:
    """``[start, end, label]`` rows in the lab format of ``chord_extractor.transcribe_midi``"""
    with open(path, "w") as f:
        for row in rows:
            f.write("\t".join(str(v) for v in row) + "\n")
