#!/usr/bin/env python
"""Time the two frozen decoders (pf_decoder): one JSON line with ms per PianoTree decode at R = 8 and R = 64, ms per chord decode at
R = 16 (median of 5 after a warm-up, hipEvents around one decode) and the launch counts.  Synthetic weights; needs a GPU."""
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from polyffusion_amd.model_sdf import ChordDecoder, PianoTreeDecoder  # noqa: E402
from polyffusion_amd.weights import synth_chord_decoder_state, synth_pianotree_decoder_state  # noqa: E402


def time_ms(fn, reps=5, warmup=2):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b))
    return statistics.median(out)


def main():
    rng = np.random.Generator(np.random.PCG64(0))
    pn = PianoTreeDecoder(max_simu_note=20).load_state_dict(synth_pianotree_decoder_state(0))
    chd = ChordDecoder(36, 256, 512, 256, 8).load_state_dict(synth_chord_decoder_state(0))
    res = {"pianotree_launches": pn.n_launches(8), "chord_launches": chd.n_launches(16)}
    for rows in (8, 64):
        z = torch.from_numpy(rng.standard_normal((rows, 512)).astype(np.float32)).cuda()
        res[f"pianotree_ms_r{rows}"] = round(time_ms(lambda: pn.decode(z)), 3)
    z = torch.from_numpy(rng.standard_normal((16, 256)).astype(np.float32)).cuda()
    res["chord_ms_r16"] = round(time_ms(lambda: chd(z, True, 0.0)), 3)
    res["device"] = torch.cuda.get_device_name(0)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
