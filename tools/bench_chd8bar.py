#!/usr/bin/env python
"""Time the chd_8bar objective: one JSON line with ms per ``Chord_8Bar.get_loss_dict`` at B = 128, n_step 32 for the force masks 0 and
all-ones (row feedback; mask 0 also under batch feedback), beside the greedy ``ChordDecoder.forward`` at the same size.  Median of 5
after a warm-up, hipEvents around 10 calls; the SCLK at the end of the run is reported with it.  Synthetic weights; needs a GPU."""
import json
import os
import statistics
import subprocess
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from polyffusion_amd import chd8bar, synth  # noqa: E402
from polyffusion_amd.weights import synth_chord_decoder_state, synth_chord_encoder_state  # noqa: E402

B, CALLS = 128, 10


def time_ms(fn, reps=5, warmup=2):
    """ms per call: hipEvents around CALLS calls, median of `reps`"""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(CALLS):
            fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) / CALLS)
    return statistics.median(out)


def sclk():
    try:
        txt = subprocess.run(["rocm-smi", "--showclocks"], capture_output=True, text=True, timeout=20).stdout
        return next((ln.split(":")[-1].strip() for ln in txt.splitlines() if "sclk" in ln.lower()), None)
    except Exception:
        return None


def main():
    p = chd8bar.CHD_8BAR
    model = chd8bar.Chord_8Bar.from_params()
    model.chord_enc.load_state_dict(synth_chord_encoder_state(0, 36, p["chd_hidden_dim"], p["chd_z_dim"]))
    model.chord_dec.load_state_dict(synth_chord_decoder_state(0, 36, p["chd_z_input_dim"], p["chd_hidden_dim"], p["chd_z_dim"]))
    chord = torch.from_numpy(synth.chords(B, 1, p["chd_n_step"])).cuda()
    batch = (None, None, chord, None)
    z = model.chord_enc.encode_mean(chord)
    dec = model.chord_dec
    res = {"batch": B, "n_step": p["chd_n_step"], "launches_greedy": dec.n_launches(B), "launches_forced_row": dec.n_launches_forced(B, "row"),
           "launches_forced_batch": dec.n_launches_forced(B, "batch")}
    res["greedy_forward_ms"] = round(time_ms(lambda: dec(z, True, 0.0)), 3)
    res["encode_dist_ms"] = round(time_ms(lambda: model.chord_enc.encode_dist(chord)), 3)
    res["loss_mask0_row_ms"] = round(time_ms(lambda: model.get_loss_dict(batch, 0, 0.0)), 3)          # rate 0: every step feeds back
    res["loss_mask1_row_ms"] = round(time_ms(lambda: model.get_loss_dict(batch, 0, 1.0)), 3)          # rate 1: every step is forced
    res["loss_mask0_batch_ms"] = round(time_ms(lambda: model.get_loss_dict(batch, 0, 0.0, feedback="batch")), 3)
    res["device"], res["sclk"] = torch.cuda.get_device_name(0), sclk()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
