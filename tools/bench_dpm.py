"""What the DPM-Solver++(2M) sampler costs and where it lands, on sdf_chd8bar with synthetic weights at batch 16.

    python tools/bench_dpm.py [--batch 16] [--reps 3] [--ref_steps 500]

prints ONE JSON line:
  * ``update_us``: microseconds per ``pf_dpm_step`` (second order, history read and written: 5 streams of n floats) beside
    ``pf_ddim_step`` (3 streams) at the same n = batch * 2 * 128 * 128, mean over 200 back-to-back launches between two events;
  * ``runs``: per sampler setting (``--dpm_steps 10 / 20`` on the logsnr grid, ``--ddim_steps 50`` uniform, eta 0), eager and as
    replays of one captured step: milliseconds per ``Experiments.predict`` call of the whole batch (median of ``--reps`` after a warm-up
    call) and per 8-bar sample, the number of denoiser evaluations, and the max-abs / RMS distance of the result from a long DDIM run
    (eta 0) on the same start noise - both solve the same probability-flow ODE, so the distance is solver error plus the two runs'
    rounding.  The long run has ``--ref_steps`` uniform steps: 500 is the longest uniform DDIM grid whose shifted time steps (1, 3, ...,
    999) stay inside the 1000-step schedule.
Synthetic weights say what the solver does on THIS denoiser; sample quality on a trained checkpoint is not measured here.  Nothing is
asserted: the numbers are recorded under profiles/ and quoted in DESIGN.md."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from polyffusion_amd import _lib, _steps, synth  # noqa: E402
from polyffusion_amd.inference_sdf import Experiments, synthetic_model  # noqa: E402
from polyffusion_amd.params import preset  # noqa: E402
from polyffusion_amd.sampler import DDIMSampler, DPMSolverSampler  # noqa: E402


def update_us(lib, n: int, launches: int = 200) -> dict:
    x, eps, hist, out = (torch.randn(n, device="cuda") for _ in range(4))
    dpm = _lib.DpmCoef(0.6, 0.8, 0.9, 0.3, -0.1, 0.8, 0.6)
    ddim = _lib.DdimCoef(0.6, 0.8, 0.85, 0.5, 0.0, 0.8, 0.6)
    calls = {"pf_dpm_step": lambda: _steps.dpm_step(lib, x, eps, out, coef=dpm, x0_prev=hist, x0_out=hist),
             "pf_ddim_step": lambda: _steps.ddim_step(lib, x, eps, out, coef=ddim)}
    res = {"n": n}
    for name, call in calls.items():
        for _ in range(20):
            call()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(launches):
            call()
        e1.record()
        torch.cuda.synchronize()
        res[name] = round(e0.elapsed_time(e1) * 1e3 / launches, 3)
    return res


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--ref_steps", type=int, default=500)
    ap.add_argument("--seed", type=int, default=1234)
    a = ap.parse_args(argv)
    _lib.require_gpu()
    p = preset("sdf_chd8bar")
    model = synthetic_model(p)
    model.ldm.eps_model.set_precision("bf16x3")
    B = a.batch
    cond = model._encode_chord(torch.from_numpy(synth.chords(B, 4242)).cuda())
    shape = (B, p.out_channels, p.img_h, p.img_w)
    noise = _steps.randn(_lib.load(), shape, "cuda", a.seed, 0, 0)

    def predict(sampler):
        return Experiments("sdf_chd8bar", p, sampler).predict(cond, uncond_scale=1.0, noise=noise)

    ref = predict(DDIMSampler(model.ldm, a.ref_steps, "uniform", 0.0, seed=a.seed, graph=True))
    settings = {"dpm10": lambda g: DPMSolverSampler(model.ldm, 10, seed=a.seed, graph=g),
                "dpm20": lambda g: DPMSolverSampler(model.ldm, 20, seed=a.seed, graph=g),
                "ddim50": lambda g: DDIMSampler(model.ldm, 50, "uniform", 0.0, seed=a.seed, graph=g)}
    runs = {}
    for name, make in settings.items():
        for graph in (False, True):
            s = make(graph)
            out = predict(s)                                   # warm-up (and the capture)
            ms = []
            for _ in range(a.reps):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                out = predict(s)
                torch.cuda.synchronize()
                ms.append((time.perf_counter() - t0) * 1e3)
            d = (out - ref).double()
            runs[f"{name}_{'graph' if graph else 'eager'}"] = {
                "evaluations": len(s.time_steps), "ms_per_batch": round(statistics.median(ms), 2),
                "ms_per_sample": round(statistics.median(ms) / B, 3), "max_abs_from_ref": float(d.abs().max()),
                "rms_from_ref": float(d.pow(2).mean().sqrt())}
    res = {"what": f"sdf_chd8bar synthetic weights, B={B}, {model.ldm.eps_model.precision}; ref = DDIM {a.ref_steps} uniform steps, eta 0",
           "ref_rms": float(ref.double().pow(2).mean().sqrt()), "ref_max_abs": float(ref.abs().max()),
           "update_us": update_us(_lib.load(), B * p.out_channels * p.img_h * p.img_w), "runs": runs}
    print(json.dumps(res))
    return 0


if __name__ == "__main__":
    sys.exit(main())
