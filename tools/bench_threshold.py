"""What clipping and dynamic thresholding of the predicted x0 cost, per call of ``pf_x0_threshold`` and per reverse step on the shape of
BASELINE config 3: sdf_chd8bar with synthetic weights, DDIM eta 0 over the whole 50-step uniform grid, scale 5, batch 32.

    python tools/bench_threshold.py [--batch 32] [--reps 3] [--out profiles/threshold_bench.json]

runs its two GPU steps as child processes, each under a time limit of its own (the second is not started when the first fails), prints
ONE JSON line and records it in ``--out``:
  * ``call_us`` (step ``kernels``): microseconds per call, mean over 200 back-to-back calls between two events, the forms taken in turn
    ``rounds`` times (the median and the spread over the rounds): the resident and the streamed form with ``stats`` as the samplers call
    them (out of place here, so that every timed call does the same work on the same inputs), mode dynamic at p = 0.995, at ``[16, 32768]`` and ``[32, 32768]``; the streamed form at ``[4, 131072]`` - four
    songs of seven half-overlapping windows (canvas 512 x 128, 2 channels); mode clip beside them; and the bytes a call has to move
    (x and eps in, eps' out: 12 bytes per element) over the time.  The rows are a roll of 0 / 1 cells noised to t = 500 with a
    prediction that is off, like the tests' - the histogram of the first digit then has a handful of occupied bins, as in a real step;
  * ``step_ms`` (step ``steps``): milliseconds per reverse step (device events around ``paint`` over all 50 steps, divided by 50) of
    three samplers in one process - ``plain`` (no option: the baseline, the launch sequence it always was), ``threshold`` (dynamic,
    p = 0.995) and ``clip`` - run round-robin ``--reps`` times after a warm-up call of each; median, spread, and each over ``plain``.
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

LIMITS = {"kernels": 240, "steps": 420}       # seconds per GPU step


def spread(v, nd=3):
    return {"median": round(statistics.median(v), nd), "min": round(min(v), nd), "max": round(max(v), nd)}


def part_kernels(a) -> dict:
    import torch
    from polyffusion_amd import _lib, _steps
    _lib.require_gpu()
    lib = _lib.load()
    beta = torch.linspace(0.00085 ** 0.5, 0.012 ** 0.5, 1000, dtype=torch.float64) ** 2
    table = _steps.x0_threshold_table(torch.cumprod(1.0 - beta, 0).float()).cuda()
    launches, rounds, res = 200, 5, []
    for rows, n, forms in ((16, 32768, ("resident", "streamed")), (32, 32768, ("resident", "streamed")), (4, 2 * 512 * 128, ("streamed",))):
        g = torch.Generator(device="cuda").manual_seed(rows + n)
        noise = torch.randn(rows, n, device="cuda", generator=g)
        ra, rb = 1.0 / table[500, 0], table[500, 1] / table[500, 0]
        x = (ra * (torch.rand(rows, n, device="cuda", generator=g) < 0.1).float() + rb * noise).contiguous()
        eps0 = (noise + 0.3 * torch.randn(rows, n, device="cuda", generator=g)).contiguous()
        t = torch.full((rows,), 500, dtype=torch.int64, device="cuda")
        calls = {}
        for mode in ("dynamic", "clip"):
            for form in forms:
                eps, stats = torch.empty_like(eps0), torch.empty(rows, 4, dtype=torch.float64, device="cuda")
                ws = _steps.x0_threshold_workspace(lib, rows, n, x.device, form)
                ws = None if ws is None else ws.clone()
                s = _lib.X0ThresholdArgs()
                s.x, s.x_row_stride, s.eps, s.eps_out, s.t, s.t_stride = x.data_ptr(), n, eps0.data_ptr(), eps.data_ptr(), t.data_ptr(), 1
                s.table, s.n_table, s.stats, s.workspace = table.data_ptr(), 1000, stats.data_ptr(), _lib.ptr(ws)
                s.workspace_bytes = 0 if ws is None else ws.numel() * 8
                s.p, s.s_max, s.lo, s.hi = 0.995, float("inf"), 0.0, 1.0
                s.mode, s.form, s.rows, s.row_elems = _lib.X0T_MODES[mode], _lib.X0T_FORMS[form], rows, n
                calls[f"{mode}_{form}"] = (s, eps, (ws, stats))
        times = {k: [] for k in calls}
        for k, (s, _, _) in calls.items():
            for _ in range(20):
                _lib.check(lib.pf_x0_threshold(C.byref(s), _lib.current_stream()), "pf_x0_threshold", lib)
        torch.cuda.synchronize()
        for _ in range(rounds):
            for k, (s, _, _) in calls.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(launches):
                    lib.pf_x0_threshold(C.byref(s), _lib.current_stream())
                e1.record()
                torch.cuda.synchronize()
                times[k].append(e0.elapsed_time(e1) * 1e3 / launches)
        same = all(torch.equal(calls[f"{m}_{forms[0]}"][1], calls[f"{m}_{f}"][1]) for m in ("dynamic", "clip") for f in forms)
        entry = {"rows": rows, "row_elems": n, "forms_agree": bool(same), "q": [round(float(v), 4) for v in calls[f"dynamic_{forms[0]}"][2][1][:2, 0].tolist()],
                 "changed": [int(v) for v in calls[f"dynamic_{forms[0]}"][2][1][:2, 3].tolist()]}
        for k, v in times.items():
            entry[k] = spread(v)
            entry[k]["GB_per_s_of_12_bytes_per_element"] = round(12.0 * rows * n / (statistics.median(v) * 1e-6) / 1e9, 1)
        res.append(entry)
    return {"device": torch.cuda.get_device_name(0), "call_us": res, "launches_per_timing": launches, "rounds": rounds}


def part_steps(a) -> dict:
    import torch
    from polyffusion_amd import _lib, _steps, synth
    from polyffusion_amd.inference_sdf import encode_conditions, synthetic_model
    from polyffusion_amd.params import preset
    from polyffusion_amd.sampler import DDIMSampler, X0Threshold
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
    variants = {"plain": {}, "threshold": dict(x0_threshold=X0Threshold("dynamic", 0.995)), "clip": dict(x0_threshold=X0Threshold("clip"))}
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
    step_ms = {name: spread(v) for name, v in times.items()}
    for name in variants:
        step_ms[name]["over_plain"] = round(step_ms[name]["median"] / step_ms["plain"]["median"], 4)
        step_ms[name]["minus_plain_us"] = round((step_ms[name]["median"] - step_ms["plain"]["median"]) * 1e3, 1)
    last = ss["threshold"].last_threshold
    return {"what": f"sdf_chd8bar synthetic weights, B={B}, {unet.precision}, DDIM eta 0, all {steps} steps of the uniform grid, scale 5, "
                    f"{a.reps} reps round-robin; ms per reverse step; sample quality not measured",
            "device": torch.cuda.get_device_name(0), "step_ms": step_ms,
            "last_step_changed_elements": [int(v) for v in last[:, 3].tolist()][:4]}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--seed", type=int, default=1234)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "threshold_bench.json"))
    ap.add_argument("--part", choices=list(LIMITS), default=None, help="run one GPU step in this process and print its JSON (what the parent starts)")
    a = ap.parse_args(argv)
    if a.part:
        print(json.dumps({"kernels": part_kernels, "steps": part_steps}[a.part](a)))
        return 0
    res = {}
    for part, limit in LIMITS.items():
        cmd = [sys.executable, os.path.abspath(__file__), "--part", part, "--batch", str(a.batch), "--reps", str(a.reps), "--seed", str(a.seed)]
        try:
            done = subprocess.run(cmd, capture_output=True, text=True, timeout=limit)
        except subprocess.TimeoutExpired:
            print(f"bench_threshold: step {part} did not finish in {limit} s; nothing more is started", file=sys.stderr)
            return 1
        if done.returncode != 0:
            sys.stderr.write(done.stderr[-4000:])
            print(f"bench_threshold: step {part} ended with status {done.returncode}; nothing more is started", file=sys.stderr)
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
