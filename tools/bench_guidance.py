"""What dual guidance costs per reverse step, on sdf_chd8bar_txt with synthetic weights at batch 16.

    python tools/bench_guidance.py [--batch 16] [--steps 10] [--reps 5] [--out profiles/dual_guidance_bench.json]

prints ONE JSON line and records it in ``--out``:
  * ``step_ms``: milliseconds per reverse step of a DDIM loop (eta 0, ``--steps`` steps of the 50-step uniform grid) for four ways of
    evaluating eps - ``none`` (scale 1: one evaluation), ``two_way_shared`` (scale 5: the reference's guidance, prefix evaluated once),
    ``three_way_shared`` (``DualScale(3, 5)``: three groups, prefix once) and ``three_way_unshared`` (the same on ``cat([x, x, x])``) - eager
    (device events around the whole loop, which ends in a synchronise) and as replays of one captured step (the sampler's own replay events).
    The variants are run round-robin ``--reps`` times after a warm-up call of each; the median is reported with the spread (min, max);
  * ``launches``: library launches per step for each - the UNet plan with its prepared prefix, the combine kernel where there is one, the
    update kernel (torch's concatenations of the few-KB context are not counted);
  * ``combine_us``: microseconds per ``pf_cfg_combine3`` (four streams of n floats) beside ``pf_cfg_combine`` (three) at the same
    n = batch * 2 * 128 * 128, mean over 200 back-to-back launches between two events;
  * ``ratios``: the three-way shared step over the two-way step and over the unshared three-way step.
Synthetic weights say what the plan costs; sample quality on a trained checkpoint is not measured here.  Nothing is asserted."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from polyffusion_amd import _lib, _steps, synth  # noqa: E402
from polyffusion_amd.inference_sdf import encode_conditions, synthetic_model  # noqa: E402
from polyffusion_amd.params import preset  # noqa: E402
from polyffusion_amd.sampler import DDIMSampler, DualScale, guidance_plan  # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def combine_us(lib, n: int, launches: int = 200) -> dict:
    e3, out = torch.randn(3 * n, device="cuda"), torch.empty(n, device="cuda")
    calls = {"pf_cfg_combine3": lambda: lib.pf_cfg_combine3(e3.data_ptr(), 3.0, 5.0, out.data_ptr(), n, _lib.current_stream()),
             "pf_cfg_combine": lambda: lib.pf_cfg_combine(e3.data_ptr(), 5.0, out.data_ptr(), n, _lib.current_stream())}
    res = {"n": n}
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
    return res


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--seed", type=int, default=1234)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "dual_guidance_bench.json"))
    a = ap.parse_args(argv)
    _lib.require_gpu()
    p = preset("sdf_chd8bar_txt")
    model = synthetic_model(p)
    unet = model.ldm.eps_model
    unet.set_precision("bf16x3")
    B = a.batch
    chd, prmat = torch.from_numpy(synth.chords(B, 4242)).cuda(), torch.from_numpy(synth.prmat(B, 4243)).cuda()
    cond, _ = encode_conditions(model, p, chd, prmat, False)
    uc = -torch.ones_like(cond)
    x = _steps.randn(_lib.load(), (B, p.out_channels, p.img_h, p.img_w), "cuda", a.seed, 0, 0)
    dual = DualScale(3.0, 5.0, model.cond_split)
    variants = {"none": (1.0, True), "two_way_shared": (5.0, True), "three_way_shared": (dual, True), "three_way_unshared": (dual, False)}

    def sampler(name, graph):
        s = DDIMSampler(model.ldm, 50, "uniform", 0.0, seed=a.seed, graph=graph)
        s.share_cfg_prefix = variants[name][1]
        return s

    def loop_ms(s, name):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        s.paint(x, cond, a.steps - 1, uncond_scale=variants[name][0], uncond_cond=uc)
        e1.record()
        torch.cuda.synchronize()
        if s.graph:                                   # the replays alone (the call also refreshes the static buffers and the prefix)
            r0, r1, n = s.last_replay
            return r0.elapsed_time(r1) / n
        return e0.elapsed_time(e1) / a.steps

    step_ms = {}
    for graph in (False, True):
        ss = {name: sampler(name, graph) for name in variants}
        for name, s in ss.items():
            loop_ms(s, name)                          # warm-up (sizes the workspace; the capture)
        times = {name: [] for name in variants}
        for _ in range(a.reps):                       # round-robin: drift of the box hits every variant alike
            for name, s in ss.items():
                times[name].append(loop_ms(s, name))
        step_ms["graph" if graph else "eager"] = {name: {"median": round(statistics.median(v), 3), "min": round(min(v), 3), "max": round(max(v), 3)}
                                                  for name, v in times.items()}
    launches = {}
    for name, (scale, share) in variants.items():
        groups = guidance_plan(cond, scale, uc)[1]
        plan = unet.n_launches(groups * B, prepared=True, shared_x=groups if (share and groups > 1) else False)
        launches[name] = {"unet": plan, "combine": int(groups > 1), "update": 1, "total": plan + int(groups > 1) + 1}
    ratios = {mode: {"three_way_shared_over_two_way_shared": round(v["three_way_shared"]["median"] / v["two_way_shared"]["median"], 4),
                     "three_way_shared_over_three_way_unshared": round(v["three_way_shared"]["median"] / v["three_way_unshared"]["median"], 4)}
              for mode, v in step_ms.items()}
    res = {"what": f"sdf_chd8bar_txt synthetic weights, B={B}, {unet.precision}, DDIM eta 0, {a.steps} steps per loop, {a.reps} reps round-robin; "
                   "ms per reverse step; sample quality not measured",
           "device": torch.cuda.get_device_name(0), "step_ms": step_ms, "launches": launches,
           "combine_us": combine_us(_lib.load(), B * p.out_channels * p.img_h * p.img_w), "ratios": ratios}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
