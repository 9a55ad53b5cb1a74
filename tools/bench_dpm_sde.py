"""What the stochastic DPM-Solver++(2M) costs beside the deterministic one.

    python tools/bench_dpm_sde.py [--out profiles/dpm_sde_bench.json] [--reps 3]

writes ONE JSON object (and prints it as one line):
  * ``update_us`` at n = 32 * 2 * 128 * 128: microseconds per ``pf_dpm_step`` (second order, history read and written), per ``pf_randn`` +
    ``pf_dpm_sde_step`` in the tensor form, and per ``pf_dpm_sde_step`` with the noise drawn in the kernel - mean over 200 back-to-back
    launches between two events, after 20 warm-up launches;
  * ``step_ms`` on sdf_chd8bar with synthetic weights at BASELINE config 3's shape (batch 16, guidance scale 5), 20 steps: milliseconds per
    reverse step of ``paint`` for eta = 0 and eta = 1, eager and as replays of one captured step (median of ``--reps`` loops after a
    warm-up loop, divided by the loop's length);
  * ``steered``: the eager eta = 1 loop on 8 groups of 4 candidates steered with ``every = 5`` (reward ``integrity``, which needs no
    chords) beside the same 32 rows unsteered.
Nothing is asserted: the numbers are recorded under profiles/ and quoted in README.md / DESIGN.md."""
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
from polyffusion_amd.inference_sdf import synthetic_model  # noqa: E402
from polyffusion_amd.params import preset  # noqa: E402
from polyffusion_amd.sampler import DPMSolverSampler, Steering  # noqa: E402


def update_us(lib, n: int, launches: int = 200) -> dict:
    x, eps, hist, out, nz = (torch.randn(n, device="cuda") for _ in range(5))
    dpm = _lib.DpmCoef(0.6, 0.8, 0.9, 0.3, -0.1, 0.8, 0.6)
    sde = _lib.DpmSdeCoef(0.6, 0.8, 0.7, 0.4, -0.1, 0.8, 0.6, 0.5)

    def tensor_form():
        _lib.check(lib.pf_randn(nz.data_ptr(), n, 1, 2, 0, _lib.current_stream()), "pf_randn", lib)
        _steps.dpm_sde_step(lib, x, eps, out, coef=sde, x0_prev=hist, x0_out=hist, noise=nz)

    calls = {"pf_dpm_step": lambda: _steps.dpm_step(lib, x, eps, out, coef=dpm, x0_prev=hist, x0_out=hist),
             "pf_randn+pf_dpm_sde_step": tensor_form,
             "pf_dpm_sde_step_rng": lambda: _steps.dpm_sde_step(lib, x, eps, out, coef=sde, x0_prev=hist, x0_out=hist, rng=(1, 2, 0))}
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


def loop_ms(sampler, x, cond, reps: int, **kw) -> float:
    t = len(sampler.time_steps) - 1
    sampler.paint(x.clone(), cond, t, **kw)                    # warm-up (and the capture)
    ms = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        sampler.paint(x.clone(), cond, t, **kw)
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ms) / (t + 1)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "dpm_sde_bench.json"))
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--seed", type=int, default=1234)
    a = ap.parse_args(argv)
    _lib.require_gpu()
    lib = _lib.load()
    p = preset("sdf_chd8bar")
    model = synthetic_model(p)
    model.ldm.eps_model.set_precision("bf16x3")

    def inputs(B):
        cond = model._encode_chord(torch.from_numpy(synth.chords(B, 4242)).cuda())
        return _steps.randn(lib, (B, p.out_channels, p.img_h, p.img_w), "cuda", a.seed, 0, 0), cond, -torch.ones_like(cond)

    x, cond, uc = inputs(16)
    step_ms = {}
    for eta in (0.0, 1.0):
        for graph in (False, True):
            s = DPMSolverSampler(model.ldm, 20, eta=eta, seed=a.seed, graph=graph)
            step_ms[f"eta{eta:g}_{'graph' if graph else 'eager'}"] = round(loop_ms(s, x, cond, a.reps, uncond_scale=5.0, uncond_cond=uc), 3)
    x, cond, uc = inputs(32)
    steered = {}
    for name, st in (("unsteered", None), ("every5", Steering(n=4, reward="integrity", every=5))):
        s = DPMSolverSampler(model.ldm, 20, eta=1.0, seed=a.seed, steering=st)
        steered[name] = round(loop_ms(s, x, cond, a.reps, uncond_scale=5.0, uncond_cond=uc), 3)
    res = {"what": f"sdf_chd8bar synthetic weights, {model.ldm.eps_model.precision}, 20 logsnr steps ({len(s.time_steps)} on the grid), guidance scale 5",
           "update_us": update_us(lib, 32 * 2 * 128 * 128), "step_ms_batch16": step_ms, "step_ms_batch32_8x4": steered}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))
    return 0


if __name__ == "__main__":
    sys.exit(main())
