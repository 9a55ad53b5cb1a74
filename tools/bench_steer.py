"""What steering by resampling costs and, on the synthetic net, what it does to the reward: per launch of the three new kernels, per reverse
step on the shape of BASELINE config 3 (sdf_chd8bar with synthetic weights, DDIM eta 1 over the whole 50-step uniform grid, scale 5, batch
32 = 8 groups of 4 candidates), and the mean final chord_f1 of the kept songs with and without ``--steer`` on the same seeds.

    python tools/bench_steer.py [--batch 32] [--reps 3] [--out profiles/steer_bench.json]

runs its three GPU steps as child processes, each under a time limit of its own (a step is not started when the one before it failed),
prints ONE JSON line and records it in ``--out``:
  * ``launch_us`` (step ``kernels``): microseconds per call, mean over 200 back-to-back calls between two events, median and spread over 5
    rounds: ``pf_x0_predict`` at ``[32, 32768]``, ``pf_steer_resample`` at 8 groups of 4 and at 1 group of 256, ``pf_rows_gather`` of two
    tensors ``[32, 32768]`` (``x`` and eps together), and the bytes each has to move over the time;
  * ``step_ms`` (step ``steps``): milliseconds per reverse step (device events around ``paint`` over all 50 steps, divided by 50) of three
    samplers in one process - ``plain`` (no steering: the baseline, the launch sequence it always was), ``every1`` (49 events) and
    ``every5`` (9 events), reward chord_f1, lambda 10 - and of ``every5_groupwise``, the same 8 groups as 8 ``paint`` calls of 4 rows, which is
    how the CLI runs ``--steer`` (a launch of one group is the same launch on any rank) - round-robin ``--reps`` times after a warm-up call of each; and the microseconds
    one event adds, ``(every1 - plain) * 50 / 49``;
  * ``reward`` (step ``reward``): ``--songs`` groups of ``--best_of`` candidates, 50 steps: the mean chord_f1 of the best candidate per
    group - what ``--best_of`` keeps of each song - without steering, with ``every=5``, ``lambda=10`` (the defaults) and with ``lambda=200``,
    ``ess=1``, the same seeds; and the mean over all candidates.  REPORTED, not asserted: the net is synthetic, so this says the mechanism concentrates the population, nothing about music.
Synthetic weights say what the launches cost; sample quality on a trained checkpoint is not measured here.  Nothing is asserted."""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

LIMITS = {"kernels": 120, "steps": 420, "reward": 300}       # seconds per GPU step


def spread(v, nd=3):
    return {"median": round(statistics.median(v), nd), "min": round(min(v), nd), "max": round(max(v), nd)}


def timed(fn, launches=200, rounds=5):
    import torch
    for _ in range(20):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(launches):
            fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) * 1e3 / launches)
    return out


def part_kernels(a) -> dict:
    import torch
    from polyffusion_amd import _lib, _steps
    _lib.require_gpu()
    lib, st = _lib.load(), _lib.current_stream
    beta = torch.linspace(0.00085 ** 0.5, 0.012 ** 0.5, 1000, dtype=torch.float64) ** 2
    table = _steps.x0_threshold_table(torch.cumprod(1.0 - beta, 0).float()).cuda()
    rows, n = a.batch, 32768
    g = torch.Generator(device="cuda").manual_seed(7)
    x, eps = torch.randn(rows, n, device="cuda", generator=g), torch.randn(rows, n, device="cuda", generator=g)
    x0, x2, e2 = torch.empty_like(x), torch.empty_like(x), torch.empty_like(x)
    t = torch.full((rows,), 500, dtype=torch.int64, device="cuda")
    pa = _lib.X0PredictArgs(x=x.data_ptr(), x_row_stride=n, eps=eps.data_ptr(), t=t.data_ptr(), t_stride=1, table=table.data_ptr(), n_table=1000,
                            x0=x0.data_ptr(), rows=rows, row_elems=n)
    res = {"x0_predict": spread(timed(lambda: lib.pf_x0_predict(C.byref(pa), st())))}
    res["x0_predict"]["GB_per_s_of_12_bytes_per_element"] = round(12.0 * rows * n / (res["x0_predict"]["median"] * 1e-6) / 1e9, 1)
    for name, groups, k in (("resample_8x4", rows // 4, 4), ("resample_1x256", 1, 256)):
        reward = torch.rand(groups * k, dtype=torch.float64, device="cuda", generator=g)
        base = torch.zeros_like(reward)
        anc, w, stats = torch.empty(groups * k, dtype=torch.int32, device="cuda"), torch.empty_like(reward), torch.empty(groups, 4, dtype=torch.float64, device="cuda")
        ra = _lib.SteerResampleArgs(reward=reward.data_ptr(), base=base.data_ptr(), lam=10.0, ess_frac=1.0, seed=1, group_offset=0, event=0,
                                    ancestors=anc.data_ptr(), weights=w.data_ptr(), stats=stats.data_ptr(), groups=groups, n=k)
        res[name] = spread(timed(lambda: lib.pf_steer_resample(C.byref(ra), st())))
    anc = torch.tensor([1, 1, 3, 0] * (rows // 4), dtype=torch.int32, device="cuda")
    ga = _lib.RowsGatherArgs()
    ga.src[0], ga.src[1], ga.dst[0], ga.dst[1], ga.row_elems[0], ga.row_elems[1] = x.data_ptr(), eps.data_ptr(), x2.data_ptr(), e2.data_ptr(), n, n
    ga.n_tensors, ga.ancestors, ga.groups, ga.n, ga.per = 2, anc.data_ptr(), rows // 4, 4, 1
    res["rows_gather_2"] = spread(timed(lambda: lib.pf_rows_gather(C.byref(ga), st())))
    res["rows_gather_2"]["GB_per_s_of_16_bytes_per_element"] = round(16.0 * rows * n / (res["rows_gather_2"]["median"] * 1e-6) / 1e9, 1)
    res["three_launches"] = round(res["x0_predict"]["median"] + res["resample_8x4"]["median"] + res["rows_gather_2"]["median"], 3)
    return {"device": torch.cuda.get_device_name(0), "shape": [rows, n], "launch_us": res, "launches_per_timing": 200, "rounds": 5}


def setup(a, B):
    import torch
    from polyffusion_amd import _lib, _steps, synth
    from polyffusion_amd.inference_sdf import encode_conditions, synthetic_model
    from polyffusion_amd.params import preset
    _lib.require_gpu()
    p = preset("sdf_chd8bar")
    model = synthetic_model(p)
    model.ldm.eps_model.set_precision("bf16x3")
    chd1 = torch.from_numpy(synth.chords(1, 4242)).cuda()                         # ONE song: every row is a candidate for it
    cond1, _ = encode_conditions(model, p, chd1, None, False)
    cond = cond1.expand(B, *cond1.shape[1:]).contiguous()
    x = _steps.randn(_lib.load(), (B, p.out_channels, p.img_h, p.img_w), "cuda", a.seed, 0, 0)
    return model, p, chd1.expand(B, *chd1.shape[1:]).contiguous(), cond, -torch.ones_like(cond), x


def part_steps(a) -> dict:
    import torch
    from polyffusion_amd.sampler import DDIMSampler, Steering
    B, steps, n = a.batch, 50, 4
    model, p, chd, cond, uc, x = setup(a, B)
    variants = {"plain": None, "every1": Steering(n=n, reward="chord", chord=chd, every=1), "every5": Steering(n=n, reward="chord", chord=chd, every=5)}
    ss = {name: DDIMSampler(model.ldm, steps, "uniform", 1.0, seed=a.seed, steering=st) for name, st in variants.items()}

    def loop_ms(s):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        s.paint(x, cond, steps - 1, uncond_scale=5.0, uncond_cond=uc)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / steps

    def groupwise_ms():                               # what the CLI does under --steer: every group a paint call of its own
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for g in range(0, B, n):
            sg = DDIMSampler(model.ldm, steps, "uniform", 1.0, seed=a.seed, sample_offset=g, steering=Steering(n=n, reward="chord", chord=chd[g: g + n], every=5))
            sg.paint(x[g: g + n].contiguous(), cond[g: g + n].contiguous(), steps - 1, uncond_scale=5.0, uncond_cond=uc[g: g + n].contiguous())
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / steps

    for s in ss.values():
        loop_ms(s)                                    # warm-up (sizes the workspace)
    groupwise_ms()
    times = {name: [] for name in list(variants) + ["every5_groupwise"]}
    for _ in range(a.reps):                           # round-robin: drift of the box hits every variant alike
        for name, s in ss.items():
            times[name].append(loop_ms(s))
        times["every5_groupwise"].append(groupwise_ms())
    step_ms = {name: spread(v) for name, v in times.items()}
    for name in times:
        step_ms[name]["over_plain"] = round(step_ms[name]["median"] / step_ms["plain"]["median"], 4)
        step_ms[name]["minus_plain_us"] = round((step_ms[name]["median"] - step_ms["plain"]["median"]) * 1e3, 1)
        step_ms[name]["events"] = 9 if name not in ss else 0 if ss[name].last_steering is None else len(ss[name].last_steering.steps)
    ev = step_ms["every1"]["events"]
    return {"what": f"sdf_chd8bar synthetic weights, B={B} = {B // n} groups of {n}, bf16x3, DDIM eta 1, all {steps} steps of the uniform grid, scale 5, reward "
                    f"chord_f1, lambda 10, {a.reps} reps round-robin; ms per reverse step; sample quality not measured",
            "device": torch.cuda.get_device_name(0), "step_ms": step_ms,
            "event_us": round((step_ms["every1"]["median"] - step_ms["plain"]["median"]) * 1e3 * steps / max(ev, 1), 1)}


def part_reward(a) -> dict:
    import torch
    from polyffusion_amd import score
    from polyffusion_amd.sampler import DDIMSampler, Steering
    n, steps = a.best_of, 50
    B = a.songs * n
    model, p, chd, cond, uc, x = setup(a, B)
    out = {}
    for name, st in (("best_of", None), ("steer", Steering(n=n, reward="chord", chord=chd, every=5, lam=10.0)),
                     ("steer_lam200_ess1", Steering(n=n, reward="chord", chord=chd, every=5, lam=200.0, ess=1.0))):
        s = DDIMSampler(model.ldm, steps, "uniform", 1.0, seed=a.seed, steering=st)
        gen = s.paint(x, cond, steps - 1, uncond_scale=5.0, uncond_cond=uc)
        f1 = score.roll_stats(gen, chd).scores()["chord_f1"].reshape(a.songs, n)
        out[name] = {"kept_mean_chord_f1": round(float(f1.max(1).values.mean()), 6), "all_mean_chord_f1": round(float(f1.mean()), 6)}
        if st is not None:
            rep = s.last_steering.report()
            out[name]["events"] = len(rep["steps"])
            out[name]["resampled_groups_per_event"] = [sum(f) for f in rep["resampled"]]
            out[name]["distinct_ancestors_per_group"] = [len(set(row)) for row in s.last_steering.lineage().tolist()]
    return {"what": f"{a.songs} groups of {n} candidates of one synthetic song, 50 DDIM steps at eta 1, scale 5, same seeds; kept = the best of each group; "
                    "reported, not asserted", "reward": out}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--seed", type=int, default=1234)
    ap.add_argument("--songs", type=int, default=8)
    ap.add_argument("--best_of", type=int, default=4)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "steer_bench.json"))
    ap.add_argument("--part", choices=list(LIMITS), default=None, help="run one GPU step in this process and print its JSON (what the parent starts)")
    a = ap.parse_args(argv)
    if a.part:
        print(json.dumps({"kernels": part_kernels, "steps": part_steps, "reward": part_reward}[a.part](a)))
        return 0
    res = {}
    for part, limit in LIMITS.items():
        cmd = [sys.executable, os.path.abspath(__file__), "--part", part, "--batch", str(a.batch), "--reps", str(a.reps), "--seed", str(a.seed),
               "--songs", str(a.songs), "--best_of", str(a.best_of)]
        try:
            done = subprocess.run(cmd, capture_output=True, text=True, timeout=limit)
        except subprocess.TimeoutExpired:
            print(f"bench_steer: step {part} did not finish in {limit} s; nothing more is started", file=sys.stderr)
            return 1
        if done.returncode != 0:
            sys.stderr.write(done.stderr[-4000:])
            print(f"bench_steer: step {part} ended with status {done.returncode}; nothing more is started", file=sys.stderr)
            return 1
        res[part] = json.loads(done.stdout.strip().splitlines()[-1])
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
