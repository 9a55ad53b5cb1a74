"""Nearest training segment of a generated roll, and how different a set of rolls is (an extension; the reference has nothing of this kind).

Two questions about a generative model, one computation: take two sets of binary piano rolls and, for every pair and every transposition
up to ``shifts`` semitones either way, the Jaccard overlap ``|qs AND c| / |qs OR c|`` of the note cells, and keep the best.  Against a
corpus of training windows the best overlap of a generated song is its ``copy_score`` (1.0: the song is a training segment, possibly
transposed); among the songs of one run it gives ``nearest_other`` and ``diversity = 1 - mean nearest_other``.

``pack_rolls`` (``pf_roll_pack``) turns images into 128-bit rows on the device, ``nearest`` / ``pairwise`` run ``pf_roll_match``
(include/pfhip.h has the definitions in full; DESIGN.md 3, "Roll matching").  Everything the device computes is integer and exact; the
ratio is formed in float64 on the device from the two integers.  A ``Corpus`` is built on the host (thresholding and ``numpy.packbits``:
a dataset tool that needs no GPU), stored once as rows with a window every ``hop`` rows, and saved as an ``.npz``.

What it is not: time shifts finer than the corpus hop, tempo or augmentation invariance, a learned embedding distance and inpainting
masks are not covered - the whole image is compared, so an inpainted song's nearest neighbour is expected to be its source.

CLI: ``python -m polyffusion_amd.rollmatch build (--from_dataset pop909|musicalion --part train --dataset_dir D --split_dir S | --from_npy
FILE... | --from_midi FILE...) --out corpus.npz [--hop 16] [--custom_round]``.
"""
from __future__ import annotations

import ctypes as C
import os
from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

from . import _lib

FORMAT_VERSION = 1
PLANES = {"onset": 0, "sounding": 1}
BAR = 16          # rows of a bar


def _plane(plane: str) -> int:
    if plane not in PLANES:
        raise ValueError(f"plane must be one of {sorted(PLANES)}, got {plane!r}")
    return PLANES[plane]


# ------------------------------------------------------------------ packing
def pack_host(prmat2c, custom_round: bool = False) -> np.ndarray:
    """``[n, 2, steps, 128]`` -> ``uint32 [2, n * steps, 4]`` on the host, word for word what ``pf_roll_pack`` writes (corpus building)."""
    x = np.asarray(prmat2c, np.float32)
    if x.ndim != 4 or x.shape[1] != 2 or x.shape[3] != 128:
        raise ValueError(f"prmat2c must be [n, 2, steps, 128], got {x.shape}")
    with np.errstate(invalid="ignore"):
        r = ((x > np.float32(0.95)) & (x < np.float32(1.05))) if custom_round else (x > np.float32(0.5))
    on = r[:, 0].reshape(-1, 128)
    both = np.stack([on, on | r[:, 1].reshape(-1, 128)])
    return np.ascontiguousarray(np.packbits(both, axis=-1, bitorder="little")).view("<u4").astype(np.uint32)


@dataclass
class PackedRolls:
    """``bits``: int32 ``[2, images * steps, 4]`` on the device (plane 0 onset, plane 1 sounding; the images' rows consecutive)."""
    bits: torch.Tensor
    images: int
    steps: int

    @property
    def rows(self) -> int:
        return self.images * self.steps

    def windows(self, steps: Optional[int] = None, hop: Optional[int] = None) -> np.ndarray:
        """Start rows (int32) of every window of ``steps`` rows at every ``hop`` rows that fits; the defaults give one window per image."""
        steps = self.steps if steps is None else int(steps)
        hop = steps if hop is None else int(hop)
        if steps < 1 or hop < 1:
            raise ValueError(f"windows: steps = {steps}, hop = {hop}")
        return np.arange(0, self.rows - steps + 1, hop, dtype=np.int32)


def pack_rolls(prmat2c: torch.Tensor, custom_round: bool = False) -> PackedRolls:
    """``prmat2c [..., 2, steps, 128]`` (leading dimensions flattened to images) on the GPU -> ``PackedRolls``; one launch, no sync."""
    _lib.require_gpu()
    lib = _lib.load()
    if prmat2c.dim() < 4 or prmat2c.shape[-3] != 2 or prmat2c.shape[-1] != 128:
        raise ValueError(f"pack_rolls: prmat2c must be [..., 2, steps, 128], got {tuple(prmat2c.shape)}")
    steps = int(prmat2c.shape[-2])
    dev = prmat2c.device if prmat2c.is_cuda else torch.device("cuda", torch.cuda.current_device())
    x = prmat2c.detach().to(device=dev, dtype=torch.float32).reshape(-1, 2, steps, 128).contiguous()
    n = int(x.shape[0])
    if n == 0 or steps == 0:
        raise ValueError(f"pack_rolls: nothing to pack in {tuple(prmat2c.shape)}")
    bits = torch.empty(2, n * steps, 4, dtype=torch.int32, device=dev)
    _lib.check(lib.pf_roll_pack(x.data_ptr(), n, steps, int(bool(custom_round)), bits.data_ptr(), _lib.current_stream()), "pf_roll_pack", lib)
    return PackedRolls(bits, n, steps)


# ------------------------------------------------------------------ the call
@dataclass
class RawMatch:
    """Device tensors of one ``pf_roll_match`` call (int32): ``index`` / ``shift`` / ``inter`` / ``union [na, topk]`` and, when asked for,
    ``tab_inter`` / ``tab_union`` / ``tab_shift [na, nb]``."""
    index: torch.Tensor
    shift: torch.Tensor
    inter: torch.Tensor
    union: torch.Tensor
    tab_inter: Optional[torch.Tensor] = None
    tab_union: Optional[torch.Tensor] = None
    tab_shift: Optional[torch.Tensor] = None


def match_windows(a_plane: torch.Tensor, a_starts: torch.Tensor, b_plane: torch.Tensor, b_starts: torch.Tensor, steps: int, shifts: int,
                  topk: int, tables: bool = False, out: Optional[RawMatch] = None, workspace: Optional[torch.Tensor] = None) -> RawMatch:
    """``pf_roll_match`` on the current stream: ``a_plane`` / ``b_plane`` int32 ``[rows, 4]`` (one plane of ``PackedRolls.bits``),
    ``a_starts`` / ``b_starts`` int32 on the same device.  ``out`` / ``workspace``: reuse (a captured call must own its buffers)."""
    _lib.require_gpu()
    lib = _lib.load()
    na, nb = int(a_starts.numel()), int(b_starts.numel())
    for name, t in (("a_plane", a_plane), ("b_plane", b_plane), ("a_starts", a_starts), ("b_starts", b_starts)):
        if t.dtype != torch.int32 or not t.is_cuda or not t.is_contiguous():
            raise ValueError(f"match_windows: {name} must be a contiguous int32 tensor on the GPU")
    dev = a_plane.device
    i32 = dict(dtype=torch.int32, device=dev)
    if out is None:
        out = RawMatch(*(torch.empty(na, topk, **i32) for _ in range(4)))
        if tables:
            out.tab_inter, out.tab_union, out.tab_shift = (torch.empty(na, nb, **i32) for _ in range(3))
    need = int(lib.pf_roll_match_workspace_bytes(na, nb, topk))
    if workspace is None:
        workspace = torch.empty(max(need, 16), dtype=torch.uint8, device=dev)
    a = _lib.RollMatchArgs(a_bits=a_plane.data_ptr(), a_starts=a_starts.data_ptr(), b_bits=b_plane.data_ptr(), b_starts=b_starts.data_ptr(),
                           na=na, nb=nb, steps=int(steps), shifts=int(shifts), topk=int(topk), reserved=0,
                           top_index=out.index.data_ptr(), top_shift=out.shift.data_ptr(), top_inter=out.inter.data_ptr(),
                           top_union=out.union.data_ptr(), tab_inter=_lib.ptr(out.tab_inter) or None, tab_union=_lib.ptr(out.tab_union) or None,
                           tab_shift=_lib.ptr(out.tab_shift) or None, workspace=workspace.data_ptr(), workspace_bytes=int(workspace.numel()))
    _lib.check(lib.pf_roll_match(C.byref(a), _lib.current_stream()), "pf_roll_match", lib)
    return out


def jaccard_of(inter: torch.Tensor, union: torch.Tensor) -> torch.Tensor:
    """inter / union in float64 where the integers live, 0.0 where union == 0"""
    ok = union != 0
    return torch.where(ok, inter.double() / torch.where(ok, union, torch.ones_like(union)).double(),
                       torch.zeros((), dtype=torch.float64, device=inter.device))


# ------------------------------------------------------------------ corpus
class Corpus:
    """Windows of ``steps`` rows into the packed rows of a set of songs, one window every ``hop`` rows of each song, none across two songs.
    Host arrays: ``bits`` uint32 ``[2, rows, 4]``, ``starts`` int32 ``[nb]``, ``song_of_window`` int32 ``[nb]``, ``row_in_song`` int32
    ``[nb]``, ``names`` (one per song)."""

    def __init__(self, bits, starts, song_of_window, row_in_song, names, steps: int, hop: int, custom_round: bool):
        self.bits = np.ascontiguousarray(bits, dtype=np.uint32)
        self.starts = np.ascontiguousarray(starts, dtype=np.int32)
        self.song_of_window = np.ascontiguousarray(song_of_window, dtype=np.int32)
        self.row_in_song = np.ascontiguousarray(row_in_song, dtype=np.int32)
        self.names = [str(n) for n in names]
        self.steps, self.hop, self.custom_round = int(steps), int(hop), bool(custom_round)
        if self.bits.ndim != 3 or self.bits.shape[0] != 2 or self.bits.shape[2] != 4:
            raise ValueError(f"Corpus: bits must be [2, rows, 4], got {self.bits.shape}")
        if not (len(self.starts) == len(self.song_of_window) == len(self.row_in_song)) or len(self.starts) == 0:
            raise ValueError("Corpus: starts, song_of_window and row_in_song must have one entry per window, and at least one")
        if self.starts.min() < 0 or int(self.starts.max()) + self.steps > self.bits.shape[1]:
            raise ValueError("Corpus: a window leaves the stored rows")
        self._device: Dict[int, tuple] = {}

    def __len__(self) -> int:
        return len(self.starts)

    @classmethod
    def from_songs(cls, songs: Sequence, names: Sequence[str], steps: int = 128, hop: int = 16, custom_round: bool = False) -> "Corpus":
        """Each song ``[segments, 2, S, 128]`` (numpy or tensor): its images' rows are one time axis.  A song shorter than ``steps`` rows is
        zero-padded to one window."""
        if len(songs) != len(names) or len(songs) == 0:
            raise ValueError(f"from_songs: {len(songs)} songs, {len(names)} names")
        if steps < 1 or hop < 1:
            raise ValueError(f"from_songs: steps = {steps}, hop = {hop}")
        bits, starts, song_of, row_in, base = [], [], [], [], 0
        for i, song in enumerate(songs):
            b = pack_host(song.detach().cpu().numpy() if isinstance(song, torch.Tensor) else song, custom_round)
            if b.shape[1] < steps:
                b = np.concatenate([b, np.zeros((2, steps - b.shape[1], 4), np.uint32)], axis=1)
            rows = np.arange(0, b.shape[1] - steps + 1, hop, dtype=np.int32)
            bits.append(b)
            starts.append(base + rows)
            song_of.append(np.full(len(rows), i, np.int32))
            row_in.append(rows)
            base += b.shape[1]
        return cls(np.concatenate(bits, axis=1), np.concatenate(starts), np.concatenate(song_of), np.concatenate(row_in), names, steps, hop,
                   custom_round)

    @classmethod
    def from_dataset(cls, dataset: str, part: str = "train", dataset_dir: Optional[str] = None, split_dir: Optional[str] = None,
                     steps: int = 128, hop: int = 16, custom_round: bool = False, use_track=(0, 1, 2), limit: Optional[int] = None) -> "Corpus":
        """The songs of one half of the dataset's split (``datasample.load_split``), each read by its sample class and cut into its
        consecutive 8-bar segments (``get_whole_song_data``).  Files without a usable segment are left out."""
        from . import datasample
        if dataset not in ("pop909", "musicalion"):
            raise ValueError(f"from_dataset: dataset {dataset!r} (pop909 or musicalion)")
        if part not in ("train", "val"):
            raise ValueError(f"from_dataset: part {part!r} (train or val)")
        split = datasample.load_split(os.path.join(split_dir or datasample.TRAIN_SPLIT_DIR, f"{dataset}.pickle"))
        files = split[0 if part == "train" else 1][:limit]
        songs, names = [], []
        for fn in files:
            if dataset == "pop909":
                sample = datasample.DataSampleNpz(fn, use_track, dataset_dir or datasample.POP909_DATA_DIR)
            else:
                sample = datasample.DataSampleNpz_Musicalion(fn, dataset_dir or datasample.MUSICALION_DATA_DIR)
            if len(sample) == 0:
                continue
            songs.append(sample.get_whole_song_data()[0].numpy())
            names.append(fn)
        if not songs:
            raise ValueError(f"from_dataset: no song with a usable segment among the {len(files)} files of {dataset} / {part}")
        return cls.from_songs(songs, names, steps, hop, custom_round)

    def save(self, path: str) -> None:
        np.savez_compressed(path, bits=self.bits, starts=self.starts, song_of_window=self.song_of_window, row_in_song=self.row_in_song,
                            names=np.array(self.names, dtype=str), steps=np.int32(self.steps), hop=np.int32(self.hop),
                            custom_round=np.bool_(self.custom_round), version=np.int32(FORMAT_VERSION))

    @classmethod
    def load(cls, path: str) -> "Corpus":
        with np.load(path, allow_pickle=False) as z:
            if "version" not in z.files or int(z["version"]) != FORMAT_VERSION:
                raise ValueError(f"{path}: corpus format version {int(z['version']) if 'version' in z.files else None}, this build reads "
                                 f"{FORMAT_VERSION}")
            return cls(z["bits"], z["starts"], z["song_of_window"], z["row_in_song"], z["names"].tolist(), int(z["steps"]), int(z["hop"]),
                       bool(z["custom_round"]))

    def where(self, window: int):
        """``(song name, bar)`` of a window; ``None`` for the index -1 of an empty slot"""
        if window < 0:
            return None
        return self.names[int(self.song_of_window[window])], int(self.row_in_song[window]) // BAR

    def on_device(self, device: torch.device):
        """``(bits int32 [2, rows, 4], starts int32 [nb])`` on the device, copied once per device"""
        key = device.index if device.index is not None else torch.cuda.current_device()
        if key not in self._device:
            self._device[key] = (torch.from_numpy(self.bits.view(np.int32)).to(device).contiguous(), torch.from_numpy(self.starts).to(device))
        return self._device[key]


# ------------------------------------------------------------------ results
def songs_report(copy_score, pick, corpus: Corpus) -> List[dict]:
    """``MatchResult.song_best``'s tensors (as they are, or gathered from several ranks) -> per song ``copy_score`` and ``nearest``: the
    song name, bar, shift, image and window of its best match (one host copy each)."""
    out = []
    for c, (window, shift, image) in zip(copy_score.tolist(), pick.tolist()):
        w = corpus.where(window)
        out.append(dict(copy_score=float(c), nearest=None if w is None else dict(song=w[0], bar=w[1], shift=int(shift), image=int(image),
                                                                                   window=int(window))))
    return out


@dataclass
class MatchResult:
    """``index`` / ``shift`` / ``inter`` / ``union``: int32 ``[queries, topk]`` on the device, best first."""
    index: torch.Tensor
    shift: torch.Tensor
    inter: torch.Tensor
    union: torch.Tensor
    corpus: Optional[Corpus] = None

    @property
    def jaccard(self) -> torch.Tensor:
        return jaccard_of(self.inter, self.union)

    def where(self) -> List[list]:
        """``(song name, bar)`` of every match (``None`` in an empty slot); one host copy"""
        return [[self.corpus.where(i) for i in row] for row in self.index.tolist()]

    def song_best(self, segments: int = 1):
        """Per song of ``segments`` consecutive queries, on the device: ``copy_score`` float64 ``[songs]`` (the maximum over its images of the
        best Jaccard, the first image on a tie) and ``pick`` int32 ``[songs, 3]`` (window, shift, image of that maximum).  No host sync."""
        n = int(self.index.shape[0])
        if segments < 1 or n % segments != 0:
            raise ValueError(f"{n} queries are not whole songs of {segments} images")
        j = self.jaccard[:, 0].reshape(-1, segments)
        best = j.max(dim=1).values
        first = (j == best[:, None]).int().argmax(dim=1)                         # argmax of a 0/1 tensor: the first maximum
        e = torch.arange(n // segments, device=j.device) * segments + first
        return best, torch.stack([self.index[e, 0], self.shift[e, 0], first.int()], dim=1)

    def songs(self, segments: int = 1) -> List[dict]:
        return songs_report(*self.song_best(segments), self.corpus)

    def report(self) -> List[list]:
        """Per query its matches, best first: jaccard, inter, union, shift, window, song, bar"""
        j, idx, sh, it, un = (t.tolist() for t in (self.jaccard, self.index, self.shift, self.inter, self.union))
        out = []
        for q in range(len(idx)):
            row = []
            for r in range(len(idx[q])):
                if idx[q][r] < 0:
                    continue
                w = self.corpus.where(idx[q][r])
                row.append(dict(jaccard=j[q][r], inter=it[q][r], union=un[q][r], shift=sh[q][r], window=idx[q][r], song=w[0], bar=w[1]))
            out.append(row)
        return out


def _as_packed(rolls, custom_round: bool) -> PackedRolls:
    return rolls if isinstance(rolls, PackedRolls) else pack_rolls(rolls, custom_round)


def nearest(queries, corpus: Corpus, shifts: int = 6, topk: int = 3, plane: str = "onset") -> MatchResult:
    """``queries`` (``[..., 2, steps, 128]`` or ``PackedRolls``), their rows cut into consecutive windows of the corpus' ``steps`` (an image
    each when the sizes agree; the two halves ``--autoreg`` returns are one window), against every window of the corpus.  The corpus'
    one-time upload, then no host synchronisation."""
    pl = _plane(plane)
    q = _as_packed(queries, corpus.custom_round)
    if q.rows % corpus.steps != 0 or (q.steps % corpus.steps != 0 and corpus.steps % q.steps != 0):
        raise ValueError(f"nearest: {q.images} images of {q.steps} steps do not cut into windows of {corpus.steps} steps, the corpus' size")
    b_bits, b_starts = corpus.on_device(q.bits.device)
    a_starts = torch.from_numpy(q.windows(corpus.steps, corpus.steps)).to(q.bits.device)
    r = match_windows(q.bits[pl], a_starts, b_bits[pl], b_starts, corpus.steps, shifts, topk)
    return MatchResult(r.index, r.shift, r.inter, r.union, corpus)


def nearest_other_of(jaccard: np.ndarray, segments: int) -> np.ndarray:
    """``jaccard [n, n]`` of the images of ``n / segments`` songs among themselves -> per song the best value against any image of any
    OTHER song (the diagonal and the song's own images excluded); 0.0 for a single song."""
    n = len(jaccard)
    if segments < 1 or n % segments != 0:
        raise ValueError(f"{n} images are not whole songs of {segments}")
    songs = n // segments
    out = np.zeros(songs, np.float64)
    for s in range(songs):
        own = np.zeros(n, bool)
        own[s * segments:(s + 1) * segments] = True
        block = jaccard[own][:, ~own]
        out[s] = block.max() if block.size else 0.0
    return out


def diversity_of(nearest_other: np.ndarray) -> float:
    return float(1.0 - np.mean(nearest_other)) if len(nearest_other) else 1.0


def pairwise(rolls, segments: int = 1, shifts: int = 0, plane: str = "onset", custom_round: bool = False, steps: Optional[int] = None) -> dict:
    """The images of a set of songs (``segments`` consecutive images each) among themselves, through the dense tables:
    ``jaccard [n, n]`` float64 (host), ``nearest_other [songs]`` and ``diversity``; ``steps``: cut the rows into windows of this size
    instead of one per image (``segments`` then counts windows).  With ``shifts > 0`` the table is the query row's
    best transposition onto the column's image and need not be symmetric."""
    pl = _plane(plane)
    p = _as_packed(rolls, custom_round)
    steps = p.steps if steps is None else int(steps)
    if p.rows % steps != 0:
        raise ValueError(f"pairwise: {p.rows} rows do not cut into windows of {steps}")
    starts = torch.from_numpy(p.windows(steps, steps)).to(p.bits.device)
    r = match_windows(p.bits[pl], starts, p.bits[pl], starts, steps, shifts, 1, tables=True)
    jac = jaccard_of(r.tab_inter, r.tab_union).cpu().numpy()
    other = nearest_other_of(jac, segments)
    return dict(jaccard=jac, shift=r.tab_shift.cpu().numpy(), nearest_other=other, diversity=diversity_of(other))


# ------------------------------------------------------------------ CLI
def make_parser():
    import argparse
    p = argparse.ArgumentParser(prog="python -m polyffusion_amd.rollmatch", description=__doc__.split("\n\n")[0])
    sub = p.add_subparsers(dest="command", required=True)
    b = sub.add_parser("build", help="write a corpus file")
    b.add_argument("--from_dataset", choices=["pop909", "musicalion"])
    b.add_argument("--part", choices=["train", "val"], default="train")
    b.add_argument("--dataset_dir")
    b.add_argument("--split_dir")
    b.add_argument("--from_npy", nargs="+", metavar="FILE", help="songs as [segments, 2, 128, 128] arrays (what inference_sdf writes)")
    b.add_argument("--from_midi", nargs="+", metavar="FILE", help="MIDI files, through midi_to_data and their 8-bar segments")
    b.add_argument("--out", required=True)
    b.add_argument("--hop", type=int, default=16)
    b.add_argument("--custom_round", action="store_true")
    return p


def build_corpus(args) -> Corpus:
    given = [k for k in ("from_dataset", "from_npy", "from_midi") if getattr(args, k)]
    if len(given) != 1:
        raise SystemExit("build: give exactly one of --from_dataset, --from_npy, --from_midi")
    if args.hop < 1:
        raise SystemExit(f"--hop {args.hop}: at least 1")
    try:
        if args.from_dataset:
            return Corpus.from_dataset(args.from_dataset, args.part, args.dataset_dir, args.split_dir, hop=args.hop, custom_round=args.custom_round)
        if args.from_npy:
            songs = [np.load(f) for f in args.from_npy]
            names = list(args.from_npy)
        else:
            from . import datasample, midi_to_data
            songs, names = [], []
            for f in args.from_midi:
                data = midi_to_data.get_data_for_single_midi(f, None)
                if data is None:
                    raise SystemExit(f"{f}: a barline does not fall on the 16th-note grid")
                songs.append(datasample.DataSample(data).get_whole_song_data()[0].numpy())
                names.append(f)
        return Corpus.from_songs(songs, names, 128, args.hop, args.custom_round)
    except (ValueError, OSError) as e:
        raise SystemExit(f"build: {e}")


def main(argv=None) -> int:
    import json
    args = make_parser().parse_args(argv)
    corpus = build_corpus(args)
    corpus.save(args.out)
    print(json.dumps(dict(out=args.out, songs=len(corpus.names), windows=len(corpus), rows=int(corpus.bits.shape[1]), steps=corpus.steps,
                          hop=corpus.hop, custom_round=corpus.custom_round)))
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
