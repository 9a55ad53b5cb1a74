"""What recognising the chords of a batch of rolls costs: ``pf_chord_recognize`` against the host path it restates.

    python tools/bench_chordrec.py [--reps 5]

prints ONE JSON line.  Per batch size 16 and 192 songs (one image of 128 steps each, with chords, default rounding):
  * ``kernel_ms``: milliseconds per ``chordrec.recognize_rolls`` call, the median of ``--reps`` timings with device events around ONE call
    (after a warm-up);
  * ``host_ms``: the host path on the same rolls, a host clock around all of it: the device->host copy, then per song ``midi.note_lists``'
    numpy part, ``midi.write_smf``, ``chord_extractor.PrettyMIDI`` and ``chord_extractor.recognize``; ``host_songs`` says how many songs were
    timed (the figure is scaled to the batch);
  * ``equal``: the labels of the timed songs agree (every song gets a note in its last step, so that its file has all 32 beats);
  * ``device``, ``sclk_mhz``: the device's name and the median average shader clock of its XCDs over the timed window.
Nothing is asserted and no threshold is set; the line is quoted in DESIGN.md."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from polyffusion_amd import _lib, chord_extractor, chordrec, midi, synth  # noqa: E402
from tools.bench_invert import ClockProbe  # noqa: E402


def one_call_ms(fn, reps: int) -> float:
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    return round(statistics.median(ms), 4)


def host_path(x: torch.Tensor, songs: int, tmp: str):
    """(seconds, label names per song) of the file path on the first ``songs`` images"""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    dur = midi.durations(x[:songs]).cpu().numpy()
    out = []
    for s in range(songs):
        step, key = np.nonzero(dur[s])
        notes = list(zip(key.tolist(), (step / 8).tolist(), np.minimum((step + dur[s][step, key]) / 8, 16.0).tolist()))
        path = os.path.join(tmp, "song.mid")
        midi.write_smf(path, [notes])
        rows = chord_extractor.recognize(chord_extractor.PrettyMIDI(path))
        out.append([label for a, b, label in rows for _ in range(int(round((b - a) * 2)))])
    return time.perf_counter() - t0, out


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--seed", type=int, default=1234)
    ap.add_argument("--host_songs", type=int, default=16, help="songs the host path is timed on (scaled to the batch)")
    a = ap.parse_args(argv)
    _lib.require_gpu()
    probe = ClockProbe(_lib.load())
    res = {"what": "pf_chord_recognize against write_smf + PrettyMIDI + recognize on the host; songs of one image [2, 128, 128], with chords",
           "device": torch.cuda.get_device_properties(0).name, "reps": a.reps}
    probe.begin()
    with tempfile.TemporaryDirectory() as tmp:
        for n in (16, 192):
            x = torch.from_numpy(synth.prmat2c_image(a.seed, n)).cuda()
            x[:, 0, -1, 60] = 1.0                                   # a note in the last step: the file then has every beat of the song
            chord = torch.from_numpy(synth.chords(n, a.seed + 1)).cuda()
            kernel = lambda: chordrec.recognize_rolls(x, 1, chord)
            names = kernel().names()
            k = min(n, a.host_songs)
            sec, host = host_path(x, k, tmp)
            res[f"songs{n}"] = {"kernel_ms": one_call_ms(kernel, a.reps), "host_ms": round(sec * 1e3 * n / k, 2), "host_songs": k,
                                "equal": all(names[s] == host[s] for s in range(k))}
    res["sclk_mhz"] = probe.end_mhz()
    print(json.dumps(res))
    return 0


if __name__ == "__main__":
    sys.exit(main())
