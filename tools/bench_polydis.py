#!/usr/bin/env python
"""Time Polydis on the HIP path: one JSON line with ms per ``reconstruct`` core (both encoders with their scale heads, then the
32-slot PianoTree decode at a 64-wide duration GRU; the MIDI file is not written) at R = 8 (a 16-bar song) and R = 64, the launch
count of the decode, and - for the same z at S = 32 - the decode alone at a duration width of 16 and of 64, whose ratio says what the
wide duration GRU costs.  Protocol of tools/bench_decoder.py: median of 5 after a warm-up, hipEvents around one call.  Synthetic
weights; needs a GPU.  No threshold: the numbers go into DESIGN.md."""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_decoder import time_ms  # noqa: E402
from polyffusion_amd import synth  # noqa: E402
from polyffusion_amd.polydis import DisentangleVAE, PtvaeDecoder  # noqa: E402
from polyffusion_amd.weights import synth_pianotree_decoder_state, synth_polydis_state  # noqa: E402


def main():
    model = DisentangleVAE.init_model().load_state_dict(synth_polydis_state(0))
    res = {"decode_launches": model.decoder.n_launches(8)}
    for rows in (8, 64):
        pr = torch.from_numpy(synth.prmat(rows // 4, 1)).reshape(-1, 32, 128).cuda()
        c = torch.from_numpy(synth.chords(rows // 4, 2)).reshape(-1, 8, 36).cuda()
        res[f"reconstruct_ms_r{rows}"] = round(time_ms(lambda: model.inference(pr, c, sample=False)), 3)
        res[f"encoders_ms_r{rows}"] = round(time_ms(lambda: model.inference_encode(pr, c)), 3)
    decs = {hd: PtvaeDecoder(dec_dur_hid_size=hd).load_state_dict(synth_pianotree_decoder_state(0, hd)) for hd in (16, 64)}
    rng = np.random.Generator(np.random.PCG64(0))
    for rows in (8, 64):
        z = torch.from_numpy(rng.standard_normal((rows, 512)).astype(np.float32)).cuda()
        for hd, dec in decs.items():
            res[f"decode_hd{hd}_ms_r{rows}"] = round(time_ms(lambda: dec.decode(z)), 3)
        res[f"hd64_over_hd16_r{rows}"] = round(res[f"decode_hd64_ms_r{rows}"] / res[f"decode_hd16_ms_r{rows}"], 3)
    res["device"] = torch.cuda.get_device_name(0)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
