"""Score generated rolls against the chords they were conditioned on (an extension; not in the reference).

``roll_stats`` is one HIP launch (``pf_roll_stats``, include/pfhip.h) over the images where the sampler left them: integer counters per
image, sounding cells per pitch class per beat, onset cells per step.  The scores below are ratios of those integers, formed in float64
with torch on the device, so they are exact functions of the image: independent of batch split, launch order and the number of GPUs.

It is a fixed statistic, not the reference's rule-based chord extractor and not the paper's metric: no chord is extracted, no voicing, no
key.  ``chord_fit``: of the sounding cells on beats that have a chord, the fraction whose pitch class is in the chord (precision).
``chord_cover``: of the chord's classes, beat by beat, the fraction that sounds at all in the beat (recall).  ``chord_f1``: their harmonic
mean.  ``bass_fit``: of the chord beats with a bass that sound, the fraction whose lowest sounding key has the bass class.  ``integrity``:
``midi.check_prmat2c_integrity``'s orphan-sustain fraction (lower is better).  ``onset_rate``: onset cells per step.  0 / 0 is 0.0.

The bass block [24:36] of a chord row is read as an ABSOLUTE pitch class by default: that is what ``midi_to_data.py`` (the ``--from_midi``
path, ref:data/midi_to_data.py:109-117) writes.  The dataset song files go through ``datasample.DataSample`` / ``chd_to_onehot``, which
copies the stored bass column as it is; which convention the files of POP909 hold is a property of those files that nothing in this
tree pins down, so ``bass_relative=True`` (``--score_bass_relative``) reads the block as an offset from the root instead.

CLI: ``python -m polyffusion_amd.score --npy FILE [--cond_npz FILE] [--bass_relative] [--chords [--lab OUT]] [--novelty_corpus FILE
[--novelty_shifts S --novelty_topk K]]`` prints one JSON line (``--novelty_corpus``: ``rollmatch.nearest`` against a corpus file);
``--chords`` adds what ``chordrec.recognize_rolls`` recognises in the roll (the reference's extractor on the device) under ``"recognized"``.
"""
from __future__ import annotations

import ctypes as C
import json
from dataclasses import dataclass
from typing import Dict, Optional, Sequence

import torch

from . import _lib

IDX = {n: i for i, n in enumerate(_lib.ROLL_COUNTERS)}
SCORES = ("chord_f1", "chord_fit", "chord_cover", "bass_fit", "integrity", "onset_rate")
RANK_BY = {"chord": ("chord_f1", True), "bass": ("bass_fit", True), "integrity": ("integrity", False), "texture": ("texture_fit", True),
           "extracted": ("chord_acc", True),      # chord_acc comes from chordrec.recognize_rolls, not from the counters above
           "novelty": ("copy_score", False)}      # copy_score comes from rollmatch.nearest: the least copied candidates are kept


def _ratio(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """a / b in float64 on int64 tensors, 0.0 where b == 0"""
    ok = b != 0
    return torch.where(ok, a.double() / torch.where(ok, b, torch.ones_like(b)).double(), torch.zeros((), dtype=torch.float64, device=a.device))


def scores_of(counters: torch.Tensor, steps: int) -> Dict[str, torch.Tensor]:
    """The derived scores of ``counters [N, 16]`` (images of ``steps`` steps): name -> float64 ``[N]`` where the counters live.
    ``chord_f1 = 2PR / (P + R)`` of ``P = chord_fit = a / b`` and ``R = chord_cover = c / d`` is evaluated as the one ratio of integers
    ``2ac / (ad + cb)``: one rounding, the same on every machine."""
    g = lambda name: counters[:, IDX[name]].to(torch.int64)
    a, b, c, d = g("SOUND_IN_CHORD"), g("SOUND_ON_CHORD"), g("CHORD_HEARD"), g("CHORD_CLASSES")
    return {
        "chord_f1": _ratio(2 * a * c, a * d + c * b),
        "chord_fit": _ratio(a, b),
        "chord_cover": _ratio(c, d),
        "bass_fit": _ratio(g("BASS_HIT"), g("BASS_BEATS")),
        "integrity": _ratio(g("N_ORPHAN"), g("N_ORPHAN") + g("N_ONSET")),
        "onset_rate": _ratio(g("N_ONSET"), torch.full_like(g("N_ONSET"), int(steps))),
    }


def report_of(counters: torch.Tensor, steps: int) -> list:
    """Per image: the scores as Python floats and the named counters as ints (one host copy)."""
    sc = {k: v.tolist() for k, v in scores_of(counters, steps).items()}
    cnt = counters.tolist()
    return [dict({k: sc[k][i] for k in SCORES}, counters={n: int(cnt[i][j]) for n, j in IDX.items()}) for i in range(len(cnt))]


@dataclass
class RollStats:
    """The three device tensors of one ``pf_roll_stats`` call (int32): ``counters [N, 16]`` (``_lib.ROLL_COUNTERS`` names the slots),
    ``chroma [N, steps / 4, 12]``, ``onsets [N, steps]``."""
    counters: torch.Tensor
    chroma: torch.Tensor
    onsets: torch.Tensor

    @property
    def steps(self) -> int:
        return int(self.onsets.shape[1])

    def counter(self, name: str) -> torch.Tensor:
        return self.counters[:, IDX[name]].to(torch.int64)

    def songs(self, segments: int) -> "RollStats":
        """Rows grouped into songs of ``segments`` consecutive images: the counters summed (lowest / highest key: over the segments that
        sound), the two tables joined along time - so that the ratios are the song's, not a mean of its segments' ratios."""
        n = self.counters.shape[0]
        if segments < 1 or n % segments != 0:
            raise ValueError(f"RollStats.songs: {n} images are not whole songs of {segments} segments")
        c = self.counters.reshape(n // segments, segments, -1).to(torch.int64)
        out = c.sum(1)
        lo, hi = c[..., IDX["LOW_KEY"]], c[..., IDX["HIGH_KEY"]]
        low = torch.where(lo >= 0, lo, torch.full_like(lo, 128)).amin(1)
        out[:, IDX["LOW_KEY"]] = torch.where(low < 128, low, torch.full_like(low, -1))
        out[:, IDX["HIGH_KEY"]] = hi.amax(1)
        return RollStats(out.to(torch.int32), self.chroma.reshape(n // segments, -1, 12), self.onsets.reshape(n // segments, -1))

    def scores(self) -> Dict[str, torch.Tensor]:
        return scores_of(self.counters, self.steps)

    def report(self) -> list:
        return report_of(self.counters, self.steps)


def roll_stats(prmat2c: torch.Tensor, chord: Optional[torch.Tensor] = None, mask: Optional[torch.Tensor] = None, *,
               custom_round: bool = False, bass_relative: bool = False) -> RollStats:
    """``prmat2c [..., 2, steps, 128]`` (any leading shape, flattened to N images) on the GPU -> ``RollStats``, one launch on the current
    stream, no synchronisation.  ``chord``: ``N * steps / 4`` rows of 36 in the images' order, in any shape - ``[N, 32, 36]`` for 128-step
    images, the same tensor for their ``[2N, 2, 64, 128]`` ``--autoreg`` halves or for canvases; ``mask``: shaped like ``prmat2c``, only cells
    whose mask is 0 count (the cells inpainting invented)."""
    _lib.require_gpu()
    lib = _lib.load()
    if prmat2c.dim() < 4 or prmat2c.shape[-3] != 2 or prmat2c.shape[-1] != 128:
        raise ValueError(f"roll_stats: prmat2c must be [..., 2, steps, 128], got {tuple(prmat2c.shape)}")
    steps = int(prmat2c.shape[-2])
    if steps <= 0 or steps % 4 != 0:
        raise ValueError(f"roll_stats: steps = {steps} is not a whole number of beats (4 steps each)")
    dev = prmat2c.device if prmat2c.is_cuda else torch.device("cuda", torch.cuda.current_device())
    x = prmat2c.detach().to(device=dev, dtype=torch.float32).reshape(-1, 2, steps, 128).contiguous()
    n, beats = int(x.shape[0]), steps // 4
    if n == 0:
        raise ValueError("roll_stats: no image")
    if chord is not None:
        if chord.numel() != n * beats * 36:
            raise ValueError(f"roll_stats: {n} images of {beats} beats need {n * beats} chord rows of 36, got {tuple(chord.shape)}")
        chord = chord.detach().to(device=x.device, dtype=torch.float32).reshape(n, beats, 36).contiguous()
    if mask is not None:
        if mask.numel() != x.numel():
            raise ValueError(f"roll_stats: the mask must be shaped like prmat2c {tuple(prmat2c.shape)}, got {tuple(mask.shape)}")
        mask = mask.detach().to(device=x.device, dtype=torch.float32).reshape(x.shape).contiguous()
    out = RollStats(torch.empty(n, _lib.ROLL_NCOUNT, dtype=torch.int32, device=x.device),
                    torch.empty(n, beats, 12, dtype=torch.int32, device=x.device), torch.empty(n, steps, dtype=torch.int32, device=x.device))
    a = _lib.RollStatsArgs(prmat2c=x.data_ptr(), chord=_lib.ptr(chord) or None, mask=_lib.ptr(mask) or None, n=n, steps=steps,
                           custom_round=int(bool(custom_round)), bass_relative=int(bool(bass_relative)),
                           counters=out.counters.data_ptr(), chroma=out.chroma.data_ptr(), onsets=out.onsets.data_ptr())
    _lib.check(lib.pf_roll_stats(C.byref(a), _lib.current_stream()), "pf_roll_stats", lib)
    return out


def texture_fit(a: RollStats, b: RollStats) -> torch.Tensor:
    """Cosine of the two ``onsets`` tables per image, float64 ``[N]``: how closely a generated roll follows the rhythm of the texture song's
    roll (the latter scored with ``chord=None``), for ``chord+txt`` models.  ``dot / sqrt(|a|^2 |b|^2)`` on exact integers; 0.0 where either is
    silent."""
    if a.onsets.shape != b.onsets.shape:
        raise ValueError(f"texture_fit: onsets of {tuple(a.onsets.shape)} against {tuple(b.onsets.shape)}")
    x, y = a.onsets.to(torch.int64), b.onsets.to(torch.int64)
    dot, nn = (x * y).sum(-1), (x * x).sum(-1) * (y * y).sum(-1)
    ok = nn != 0
    return torch.where(ok, dot.double() / torch.where(ok, nn, torch.ones_like(nn)).double().sqrt(), torch.zeros((), dtype=torch.float64, device=x.device))


def rank(scores: Sequence[float], keep: int, descending: bool = True) -> list:
    """Indices of the best ``keep`` scores, best first.  Host code, stable: ties go to the lower index."""
    v = [float(s) for s in scores]
    if not 0 <= keep <= len(v):
        raise ValueError(f"rank: keep = {keep} of {len(v)} scores")
    return sorted(range(len(v)), key=lambda i: ((-v[i]) if descending else v[i], i))[:keep]


def main(argv=None) -> int:
    from argparse import ArgumentParser

    import numpy as np
    p = ArgumentParser(description="score a generated piano roll (.npy of inference_sdf) against chords")
    p.add_argument("--npy", required=True, help="[B, 2, 128, 128] piano roll (or [2B, 2, 64, 128] --autoreg halves)")
    p.add_argument("--cond_npz", help="npz with the array chord [B, 32, 36] the roll was conditioned on; without it the chord-free numbers")
    p.add_argument("--bass_relative", action="store_true", help="read the bass block of a chord row as an offset from the root")
    p.add_argument("--chords", action="store_true", help="also recognise the chords of the roll (polyffusion_amd.chordrec: the rule of --from_midi, "
                   "all images one song) and, with --cond_npz, compare them with its chords: a \"recognized\" key in the JSON line")
    p.add_argument("--lab", metavar="OUT", help="with --chords: write the recognised chords as start<TAB>end<TAB>label lines (transcribe_midi's format)")
    p.add_argument("--novelty_corpus", metavar="FILE", help="a corpus file of python -m polyffusion_amd.rollmatch build: adds the roll's "
                   "copy_score (best Jaccard overlap of an image's onset cells with any corpus window under transposition), where it was found "
                   "and the matches of every image under \"novelty\"")
    p.add_argument("--novelty_shifts", type=int, default=6, metavar="S", help="transpositions of up to S semitones either way (0..15, default 6)")
    p.add_argument("--novelty_topk", type=int, default=3, metavar="K", help="matches kept per image (1..8, default 3)")
    args = p.parse_args(argv)
    if args.lab and not args.chords:
        raise SystemExit("--lab belongs to --chords, which was not given")
    if not args.novelty_corpus and (args.novelty_shifts != 6 or args.novelty_topk != 3):
        raise SystemExit("--novelty_shifts / --novelty_topk belong to --novelty_corpus, which was not given")
    if not (0 <= args.novelty_shifts <= _lib.ROLL_MATCH_MAX_SHIFTS and 1 <= args.novelty_topk <= _lib.ROLL_MATCH_MAX_TOPK):
        raise SystemExit(f"--novelty_shifts 0..{_lib.ROLL_MATCH_MAX_SHIFTS}, --novelty_topk 1..{_lib.ROLL_MATCH_MAX_TOPK}")
    x = torch.from_numpy(np.load(args.npy)).float()
    chord = None
    if args.cond_npz:
        with np.load(args.cond_npz) as z:
            if "chord" not in z:
                raise SystemExit(f"{args.cond_npz} holds no chord array")
            chord = torch.from_numpy(z["chord"]).float()
        rows = x.shape[0] * x.shape[-2] // 4
        chord = chord.reshape(-1, 36)
        if chord.shape[0] < rows:
            raise SystemExit(f"{args.cond_npz}: {chord.shape[0]} chord rows for a roll of {rows} beats")
        chord = chord[:rows]
    if not torch.cuda.is_available():
        raise SystemExit("polyffusion_amd.score needs an AMD GPU (no CPU fallback on this path)")
    song = roll_stats(x.cuda(), None if chord is None else chord.cuda(), bass_relative=args.bass_relative).songs(x.shape[0]).report()[0]
    if args.chords:
        from . import chordrec
        try:
            rec = chordrec.recognize_rolls(x.cuda(), x.shape[0], None if chord is None else chord.cuda(), bass_relative=args.bass_relative)
        except ValueError as e:
            raise SystemExit(str(e))
        song["recognized"] = dict(rec.report()[0], path_score=float(rec.path_score[0]), lab=[[float(a), float(b), n] for a, b, n in rec.lab_rows(0)])
        if args.lab:
            chordrec.write_lab(args.lab, rec.lab_rows(0))
    if args.novelty_corpus:
        from . import rollmatch
        try:
            corpus = rollmatch.Corpus.load(args.novelty_corpus)
            m = rollmatch.nearest(x.cuda(), corpus, args.novelty_shifts, args.novelty_topk)
        except (OSError, ValueError, KeyError) as e:
            raise SystemExit(f"--novelty_corpus {args.novelty_corpus}: {e}")
        song.update(m.songs(int(m.index.shape[0]))[0])
        song["novelty"] = dict(corpus=args.novelty_corpus, shifts=args.novelty_shifts, topk=args.novelty_topk, plane="onset", matches=m.report())
    print(json.dumps(dict(song, file=args.npy, images=int(x.shape[0]), steps=int(x.shape[-2]), chords=args.cond_npz,
                          bass_relative=bool(args.bass_relative))))
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
