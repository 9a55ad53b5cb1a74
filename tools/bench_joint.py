"""What joining the segments of a song costs per reverse step: all 2B-1 half-overlapping windows in ONE loop (``--joint``) against the 2B-1
autoregressive runs (``--autoreg``), on sdf_chd8bar with synthetic weights, one song of B = 2, 4, 8 segments.

    python tools/bench_joint.py [--steps 10] [--reps 5] [--uncond_scale 1.0] [--out profiles/joint_bench.json]

prints ONE JSON line and records it in ``--out``:
  * ``step_ms``: milliseconds per reverse step index of a DDIM loop (eta 0, ``--steps`` steps of the 50-step uniform grid) for a song of B
    segments - ``joint``: ``Experiments.predict_joint``, one ``paint()`` on a canvas of 128 B rows whose denoiser batch is 2B-1;
    ``autoreg``: ``Experiments.predict_songs``, the 2B-1 ``paint()`` calls at batch 1 SUMMED - eager (device events around every ``paint()``,
    which includes its hoisted prefix) and as replays of one captured step (the sampler's own replay events, summed likewise).  The variants
    are run round-robin ``--reps`` times after a warm-up call of each; the median is reported with the spread (min, max);
  * ``launches``: library launches per step index for each - the UNet plan with its prepared prefix, split and merge (joint) or the
    combine kernel where guidance needs one (autoreg), the update kernel - the autoregressive figure times its 2B-1 runs;
  * ``window_us``: microseconds per ``pf_window_split`` and per ``pf_window_merge`` with 1 and 2 groups at the B = 8 geometry (15 windows of
    128 x 128, 2 channels), mean over 200 back-to-back launches between two events;
  * ``ratios``: the autoregressive step over the joint step.
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
from polyffusion_amd.inference_sdf import Experiments, encode_conditions, synthetic_model  # noqa: E402
from polyffusion_amd.params import preset  # noqa: E402
from polyffusion_amd.sampler import DDIMSampler, WindowPlan, guidance_plan  # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEGMENTS = (2, 4, 8)


def window_us(lib, plan: WindowPlan, channels: int, width: int, launches: int = 200) -> dict:
    rows = plan.n_windows
    canvas = torch.randn(1, channels, plan.canvas_h, width, device="cuda")
    e2 = torch.randn(2 * rows, channels, plan.win_h, width, device="cuda")
    e1 = e2[:rows].contiguous()
    w = torch.from_numpy(plan.weights()).cuda()
    out = torch.empty_like(canvas)
    calls = {"pf_window_split": lambda: _steps.window_split(lib, canvas, plan.n_windows, plan.stride, plan.win_h),
             "pf_window_merge_groups1": lambda: _steps.window_merge(lib, e1, w, 1, plan.n_windows, plan.stride, 1, (), out=out),
             "pf_window_merge_groups2": lambda: _steps.window_merge(lib, e2, w, 1, plan.n_windows, plan.stride, 2, (5.0,), out=out)}
    res = {"windows": rows, "window_floats": rows * channels * plan.win_h * width, "canvas_floats": canvas.numel()}
    for name, call in calls.items():
        for _ in range(20):
            call()
        e0, e1_ = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(launches):
            call()
        e1_.record()
        torch.cuda.synchronize()
        res[name] = round(e0.elapsed_time(e1_) * 1e3 / launches, 3)
    return res


def timed(s, steps: int) -> list:
    """Wrap ``s.paint`` so that every call leaves (start event, end event, steps) in the returned list: around the call (eager), or the
    sampler's own events around its replays (captured)."""
    spans, paint = [], s.paint

    def wrapped(*args, **kw):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = paint(*args, **kw)
        e1.record()
        spans.append(s.last_replay if s.graph else (e0, e1, steps))
        return out

    s.paint = wrapped
    return spans


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--seed", type=int, default=1234)
    ap.add_argument("--uncond_scale", type=float, default=1.0)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "joint_bench.json"))
    a = ap.parse_args(argv)
    _lib.require_gpu()
    p = preset("sdf_chd8bar")
    model = synthetic_model(p)
    unet = model.ldm.eps_model
    unet.set_precision("bf16x3")
    conds = {}
    for B in SEGMENTS:
        chd = torch.from_numpy(synth.chords(B, 4242)).cuda()
        cond, cond_mid = encode_conditions(model, p, chd, None, True)
        conds[B] = (cond.unsqueeze(0).contiguous(), cond_mid.unsqueeze(0).contiguous())
    variants = [(B, mode) for B in SEGMENTS for mode in ("joint", "autoreg")]

    def run(ex, spans, B, mode):
        del spans[:]
        cond, cond_mid = conds[B]
        (ex.predict_joint if mode == "joint" else ex.predict_songs)(cond, cond_mid, a.uncond_scale)
        torch.cuda.synchronize()
        assert len(spans) == (1 if mode == "joint" else 2 * B - 1)
        return sum(e0.elapsed_time(e1) / n for e0, e1, n in spans)          # ms per step index, the runs of the song summed

    step_ms = {}
    for graph in (False, True):
        exs = {}
        for v in variants:
            s = DDIMSampler(model.ldm, 50, "uniform", 0.0, seed=a.seed, graph=graph)
            exs[v] = (Experiments(p.model_name, p, s, t_idx=a.steps - 1), timed(s, a.steps))
        for v, (ex, spans) in exs.items():
            run(ex, spans, *v)                        # warm-up (sizes the workspace; the capture)
        times = {v: [] for v in variants}
        for _ in range(a.reps):                       # round-robin: drift of the box hits every variant alike
            for v, (ex, spans) in exs.items():
                times[v].append(run(ex, spans, *v))
        step_ms["graph" if graph else "eager"] = {f"B{B}_{mode}": {"median": round(statistics.median(t), 3), "min": round(min(t), 3), "max": round(max(t), 3)}
                                                  for (B, mode), t in times.items()}
    launches = {}
    groups = guidance_plan(conds[2][0][0], a.uncond_scale, -torch.ones_like(conds[2][0][0]))[1]
    for B in SEGMENTS:
        wn = 2 * B - 1
        shared = groups if groups > 1 else False
        joint = unet.n_launches(groups * wn, prepared=True, shared_x=shared)
        one = unet.n_launches(groups, prepared=True, shared_x=shared)
        launches[f"B{B}_joint"] = {"unet": joint, "split": 1, "merge": 1, "update": 1, "total": joint + 3}
        launches[f"B{B}_autoreg"] = {"runs": wn, "unet": one, "combine": int(groups > 1), "update": 1, "total": wn * (one + int(groups > 1) + 1)}
    ratios = {mode: {f"B{B}_autoreg_over_joint": round(v[f"B{B}_autoreg"]["median"] / v[f"B{B}_joint"]["median"], 3) for B in SEGMENTS}
              for mode, v in step_ms.items()}
    res = {"what": f"sdf_chd8bar synthetic weights, one song of B segments, {unet.precision}, uncond_scale {a.uncond_scale}, DDIM eta 0, "
                   f"{a.steps} steps per loop, {a.reps} reps round-robin; ms per reverse step index (autoreg: its 2B-1 runs summed); "
                   "sample quality not measured",
           "device": torch.cuda.get_device_name(0), "step_ms": step_ms, "launches": launches,
           "window_us": window_us(_lib.load(), WindowPlan(15, 64, 128), p.out_channels, p.img_w), "ratios": ratios}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
