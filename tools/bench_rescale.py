"""What guidance rescale and a guidance interval cost or save per reverse step, on the shape of BASELINE config 3: sdf_chd8bar with synthetic
weights, DDIM eta 0 over the whole 50-step uniform grid, scale 5, batch 32.

    python tools/bench_rescale.py [--batch 32] [--reps 3] [--out profiles/rescale_bench.json]

prints ONE JSON line and records it in ``--out``:
  * ``kernel_us``: microseconds per ``pf_cfg_rescale`` (its two launches) beside ``pf_cfg_combine`` on the same ``[2][batch][32768]`` tensors,
    mean over 200 back-to-back calls between two events, with the ratio and the ratio the bytes moved predict: the plain combine moves
    (G + 1) * n floats, the rescale reads the G groups twice and writes once, (2G + 1) * n - 5 / 3 at G = 2 - plus one launch;
  * ``step_ms``: milliseconds per reverse step (device events around ``paint`` over all 50 steps, which ends in a synchronise, divided by 50)
    of four samplers in one process - ``plain`` (no flags: the baseline to compare against), ``rescale`` (phi 0.7), ``interval``
    (fractions 0.2 .. 0.8 of the schedule: time steps 200 .. 799, which holds 30 of the grid's 50 steps) and ``both`` - run round-robin
    ``--reps`` times after a warm-up call of each; the median with the spread (min, max), and each over ``plain``;
  * ``guided_steps``: how many of the 50 steps the interval guides.
Synthetic weights say what the launches cost; sample quality on a trained checkpoint is not measured here.  Nothing is asserted."""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from polyffusion_amd import _lib, _steps, synth  # noqa: E402
from polyffusion_amd.inference_sdf import encode_conditions, synthetic_model  # noqa: E402
from polyffusion_amd.params import preset  # noqa: E402
from polyffusion_amd.sampler import DDIMSampler, guidance_interval_from_fractions  # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def kernel_us(lib, rows: int, row_elems: int, launches: int = 200) -> dict:
    n = rows * row_elems
    e2, out = torch.randn(2 * n, device="cuda"), torch.empty(n, device="cuda")
    ws = _steps.cfg_rescale_workspace(lib, rows, row_elems, "cuda")
    a = _lib.CfgRescaleArgs()
    a.epsg, a.eps, a.workspace, a.workspace_bytes = e2.data_ptr(), out.data_ptr(), ws.data_ptr(), ws.numel() * 8
    a.phi, a.s1, a.groups, a.rows, a.row_elems = 0.7, 5.0, 2, rows, row_elems
    calls = {"pf_cfg_rescale": lambda: lib.pf_cfg_rescale(C.byref(a), _lib.current_stream()),
             "pf_cfg_combine": lambda: lib.pf_cfg_combine(e2.data_ptr(), 5.0, out.data_ptr(), n, _lib.current_stream())}
    res = {"rows": rows, "row_elems": row_elems}
    for name, call in calls.items():
        for _ in range(20):
            _lib.check(call(), name)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(launches):
            call()
        e1.record()
        torch.cuda.synchronize()
        res[name] = round(e0.elapsed_time(e1) * 1e3 / launches, 3)
    res["ratio"] = round(res["pf_cfg_rescale"] / res["pf_cfg_combine"], 3)
    res["ratio_expected_from_bytes"] = round(5 / 3, 3)
    return res


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--seed", type=int, default=1234)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "rescale_bench.json"))
    a = ap.parse_args(argv)
    _lib.require_gpu()
    p = preset("sdf_chd8bar")
    model = synthetic_model(p)
    unet = model.ldm.eps_model
    unet.set_precision("bf16x3")
    B, steps = a.batch, 50
    chd, prmat = torch.from_numpy(synth.chords(B, 4242)).cuda(), torch.from_numpy(synth.prmat(B, 4243)).cuda()
    cond, _ = encode_conditions(model, p, chd, prmat, False)
    uc = -torch.ones_like(cond)
    x = _steps.randn(_lib.load(), (B, p.out_channels, p.img_h, p.img_w), "cuda", a.seed, 0, 0)
    interval = guidance_interval_from_fractions(0.2, 0.8, model.ldm.n_steps)
    variants = {"plain": {}, "rescale": dict(guidance_rescale=0.7), "interval": dict(guidance_interval=interval),
                "both": dict(guidance_rescale=0.7, guidance_interval=interval)}
    ss = {name: DDIMSampler(model.ldm, steps, "uniform", 0.0, seed=a.seed, **kw) for name, kw in variants.items()}

    def loop_ms(s):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        s.paint(x, cond, steps - 1, uncond_scale=5.0, uncond_cond=uc)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / steps

    for s in ss.values():
        loop_ms(s)                                    # warm-up (sizes the workspace)
    times = {name: [] for name in variants}
    for _ in range(a.reps):                           # round-robin: drift of the box hits every variant alike
        for name, s in ss.items():
            times[name].append(loop_ms(s))
    step_ms = {name: {"median": round(statistics.median(v), 3), "min": round(min(v), 3), "max": round(max(v), 3)} for name, v in times.items()}
    for name in variants:
        step_ms[name]["over_plain"] = round(step_ms[name]["median"] / step_ms["plain"]["median"], 4)
    guided = int(sum(ss["interval"].guided_at(t) for t in ss["interval"].time_steps[:steps]))
    res = {"what": f"sdf_chd8bar synthetic weights, B={B}, {unet.precision}, DDIM eta 0, all {steps} steps of the uniform grid, scale 5, "
                   f"{a.reps} reps round-robin; ms per reverse step; sample quality not measured",
           "device": torch.cuda.get_device_name(0), "interval": list(interval), "guided_steps": guided, "step_ms": step_ms,
           "kernel_us": kernel_us(_lib.load(), B, p.out_channels * p.img_h * p.img_w)}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
