"""What scoring a batch of rolls costs: ``pf_roll_stats`` against the same counters formed by a torch expression on the device.

    python tools/bench_score.py [--reps 5]

prints ONE JSON line.  Per batch size N = 16 and N = 256 (images of 128 steps, with chords, no mask, default rounding):
  * ``kernel_us`` / ``torch_us``: microseconds per ``score.roll_stats`` call / per evaluation of ``torch_counters`` below, the median of
    ``--reps`` timings with device events around ONE call (after a warm-up); at this size that is mostly the cost of getting one launch -
    or the few dozen launches of the torch expression - through the runtime;
  * ``kernel_us_back_to_back`` / ``torch_us_back_to_back``: the same call 200 times between two events, over 200: what it costs in a stream
    that is kept busy;
  * ``bytes``: what one call has to read (images and chords) and write; ``equal``: the torch expression gave the kernel's counters;
  * ``device``, ``sclk_mhz``: the device's name and the median average shader clock of its XCDs over the timed window.
Nothing is asserted and no threshold is set: the torch figure is the yardstick the kernel has to beat to earn its place, and the line is
quoted in DESIGN.md."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from polyffusion_amd import _lib, score, synth  # noqa: E402
from tools.bench_invert import ClockProbe  # noqa: E402

I = score.IDX


def torch_counters(x: torch.Tensor, chord: torch.Tensor) -> torch.Tensor:
    """The 14 counters of ``pf_roll_stats`` (no mask, default rounding, absolute bass) as torch operations where the tensors live:
    ``x [N, 2, S, 128]``, ``chord [N, S / 4, 36]`` -> int64 ``[N, 16]``."""
    N, _, S, K = x.shape
    B = S // 4
    on, sus = x[:, 0] > 0.5, x[:, 1] > 0.5
    snd = on | sus
    occ = (x[:, 0] > 0.5) | (x[:, 0] < -0.5) | (x[:, 1] > 0.5) | (x[:, 1] < -0.5)
    prev = torch.zeros_like(occ)
    prev[:, 1:] = occ[:, :-1]
    orphan = sus & ~prev
    onehot = (torch.arange(K, device=x.device)[:, None] % 12 == torch.arange(12, device=x.device)[None, :]).to(torch.float32)
    # counts of at most 4 * 11 per (beat, class): exact in float32, so the class sums can go through a matrix product
    per_beat = lambda cells: (cells.reshape(N, B, 4, K).sum(2).to(torch.float32) @ onehot).to(torch.int64)
    chroma, on_chroma = per_beat(snd), per_beat(on)
    C = chord[..., 12:24] > 0.5
    nC = C.sum(-1)
    cb = nC > 0
    bass_block = chord[..., 24:36]
    bass, has_bass = bass_block.argmax(-1), (bass_block > 0).any(-1)
    beat_keys = snd.reshape(N, B, 4, K).any(2)
    sounds = beat_keys.any(-1)
    lowest = beat_keys.to(torch.uint8).argmax(-1)
    bb = cb & has_bass & sounds
    keys = snd.any(1)
    any_key = keys.any(-1)
    out = torch.zeros(N, _lib.ROLL_NCOUNT, dtype=torch.int64, device=x.device)
    out[:, I["N_ONSET"]] = on.sum((1, 2))
    out[:, I["N_SOUNDING"]] = snd.sum((1, 2))
    out[:, I["N_ORPHAN"]] = orphan.sum((1, 2))
    out[:, I["CHORD_BEATS"]] = cb.sum(-1)
    out[:, I["SOUND_ON_CHORD"]] = (chroma.sum(-1) * cb).sum(-1)
    out[:, I["SOUND_IN_CHORD"]] = (chroma * C).sum((1, 2))
    out[:, I["ONSET_IN_CHORD"]] = (on_chroma * C).sum((1, 2))
    out[:, I["ONSET_ON_CHORD"]] = (on_chroma.sum(-1) * cb).sum(-1)
    out[:, I["CHORD_CLASSES"]] = nC.sum(-1)
    out[:, I["CHORD_HEARD"]] = ((chroma > 0) & C).sum((1, 2))
    out[:, I["BASS_BEATS"]] = bb.sum(-1)
    out[:, I["BASS_HIT"]] = (bb & (lowest % 12 == bass)).sum(-1)
    k8 = keys.to(torch.uint8)
    out[:, I["LOW_KEY"]] = torch.where(any_key, k8.argmax(-1), torch.full_like(nC[:, 0], -1))
    out[:, I["HIGH_KEY"]] = torch.where(any_key, K - 1 - k8.flip(-1).argmax(-1), torch.full_like(nC[:, 0], -1))
    return out


def one_call_us(fn, reps: int) -> float:
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    us = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        us.append(e0.elapsed_time(e1) * 1e3)
    return round(statistics.median(us), 2)


def back_to_back_us(fn, calls: int = 200) -> float:
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return round(e0.elapsed_time(e1) * 1e3 / calls, 2)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--seed", type=int, default=1234)
    a = ap.parse_args(argv)
    _lib.require_gpu()
    probe = ClockProbe(_lib.load())
    res = {"what": "pf_roll_stats against a torch expression of the same counters; images [N, 2, 128, 128] with chords, no mask",
           "device": torch.cuda.get_device_properties(0).name, "reps": a.reps}
    probe.begin()
    for n in (16, 256):
        x = torch.from_numpy(synth.prmat2c_image(a.seed, n)).cuda()
        chord = torch.from_numpy(synth.chords(n, a.seed + 1)).cuda()
        kernel, expr = (lambda: score.roll_stats(x, chord)), (lambda: torch_counters(x, chord))
        got, want = kernel().counters.to(torch.int64), expr()
        res[f"N{n}"] = {"kernel_us": one_call_us(kernel, a.reps), "torch_us": one_call_us(expr, a.reps),
                        "kernel_us_back_to_back": back_to_back_us(kernel), "torch_us_back_to_back": back_to_back_us(expr),
                        "bytes": int(4 * (x.numel() + chord.numel() + n * (16 + 32 * 12 + 128))), "equal": bool(torch.equal(got, want))}
    res["sclk_mhz"] = probe.end_mhz()
    print(json.dumps(res))
    return 0


if __name__ == "__main__":
    sys.exit(main())
