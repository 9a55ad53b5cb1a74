#!/usr/bin/env python
"""What one evaluation of the training objective costs at B = 16 on sdf_chd8bar (seeded synthetic weights).  One JSON line with three
times, each the median of `--windows` windows of `--steps` evaluations (HIP events) after `--warmup` evaluations:

  loss_ms      LatentDiffusion.loss with library noise: pf_qsample_rows (noise drawn in the kernel) + UNetModel.forward + pf_mse_rows (noise
               drawn again in the kernel, two launches) + the mean of 16 doubles
  forward_ms   the bare UNetModel.forward at the same batch
  composed_ms  the same loss put together from what the library offered before these kernels: pf_randn, one pf_axpby per distinct t (rows
               gathered and scattered with torch indexing), the forward, and torch for (noise - eps) ** 2 and the mean

and the differences / the ratio.  The expectation this measures: the loss costs the forward plus two small launches."""
from __future__ import annotations

import argparse
import json
import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from bench import _median  # noqa: E402
from polyffusion_amd import _lib, _steps, synth  # noqa: E402
from polyffusion_amd.inference_sdf import synthetic_model  # noqa: E402
from polyffusion_amd.params import preset  # noqa: E402


def timed(fn, steps, warmup, windows):
    for _ in range(warmup):
        fn()
    ms = []
    for _ in range(max(1, windows)):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(steps):
            out = fn()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1) / steps)
    assert torch.isfinite(out).all().item(), "non-finite result"
    return _median(ms), ms


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--precision", choices=("f32", "bf16x3", "f16x3"), default="bf16x3")
    args = ap.parse_args(argv)
    _lib.require_gpu()
    params = preset("sdf_chd8bar")
    model = synthetic_model(params, 0, x3="f16" if args.precision == "f16x3" else None)
    ldm, unet = model.ldm, model.ldm.eps_model
    unet.set_precision(args.precision)
    lib, B = unet._lib, args.batch
    x0 = torch.from_numpy(synth.prmat2c_image(1, B)).float().cuda()
    cond = model._encode_chord(torch.from_numpy(synth.chords(B, 100)).cuda())
    t_host = _steps.time_steps(None, B, ldm.n_steps, 0, "cpu")
    t = t_host.cuda()
    sa, sb = _steps.sqrt_tables(ldm.alpha_bar, "cpu")
    groups = [(torch.nonzero(t_host == v).flatten().cuda(), float(sa[v]), float(sb[v])) for v in sorted(set(t_host.tolist()))]
    xt_fixed = ldm.q_sample(x0, t, seed=0, draw=0)

    def loss():
        return ldm.loss(x0, cond, t=t, seed=0, draw=0)

    def forward():
        return unet(xt_fixed, t, cond)

    def composed():
        noise = _steps.randn(lib, x0.shape, x0.device, 0, 0, 0)
        xt = torch.empty_like(x0)
        for idx, a, b in groups:
            xt[idx] = _steps.axpby(lib, x0[idx], noise[idx], a, b)
        eps = unet(xt, t, cond)
        return ((noise - eps) ** 2).mean()

    a, b = float(loss()), float(composed())
    assert abs(a - b) <= 1e-5 * abs(a), (a, b)      # the same number up to the reduction's rounding
    res = {k: timed(f, args.steps, args.warmup, args.windows) for k, f in (("loss", loss), ("forward", forward), ("composed", composed))}
    lo, fw, co = (res[k][0] for k in ("loss", "forward", "composed"))
    print(json.dumps({
        "workload": "validation_loss", "model": params.model_name, "batch": B, "precision": unet.precision, "distinct_t": len(groups),
        "loss_ms": round(lo, 4), "forward_ms": round(fw, 4), "composed_ms": round(co, 4),
        "loss_minus_forward_ms": round(lo - fw, 4), "composed_minus_forward_ms": round(co - fw, 4), "loss_over_composed": round(lo / co, 4),
        "evaluations_per_s": round(1e3 / lo, 2), "loss": a,
        "window_ms": {k: [round(v, 4) for v in res[k][1]] for k in res},
    }))


if __name__ == "__main__":
    main()
