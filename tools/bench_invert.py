"""What exact DDIM inversion costs and how far its fixed-point iteration gets, on sdf_chd8bar with synthetic weights at batch 16.

    python tools/bench_invert.py [--batch 16] [--steps 50] [--iters 3] [--reps 3]

prints ONE JSON line:
  * ``update_us``: microseconds per ``pf_invert_step`` without and with the fused residual (the second is two launches: the update with
    its per-chunk partials, then the in-order finish) at n = batch * 2 * 128 * 128, mean over 200 back-to-back launches between two events;
  * ``ms_per_invert_step`` eager and as replays of one captured step (one upward step = ``--iters`` denoiser evaluations and updates) and
    ``ms_per_paint_step`` (one evaluation and ``pf_ddim_step``) on the same sampler, guidance 1: a whole loop's wall time (median of
    ``--reps`` after a warm-up call) over its steps;
  * ``device`` and ``sclk_mhz_invert_*``: the device's name and the median average shader clock of its XCDs over the timed inversions;
  * ``residual``: per guidance scale (1 and 5) the relative residual |x_K - x_K-1| / |x_K| of the LAST iterate - its largest and median
    value over all steps and rows - and the round trip max |paint(invert(x)) - x| on a synthetic piano roll.
Synthetic weights say what the iteration does on THIS denoiser; how it contracts on a trained checkpoint is not measured here.  Nothing
is asserted: the line is quoted in DESIGN.md."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from polyffusion_amd import _lib, _steps, synth  # noqa: E402
from polyffusion_amd.inference_sdf import synthetic_model  # noqa: E402
from polyffusion_amd.params import preset  # noqa: E402
from polyffusion_amd.sampler import DDIMSampler  # noqa: E402


def update_us(lib, rows: int, row_elems: int, launches: int = 200) -> dict:
    y, eps, out = (torch.randn(rows, row_elems, device="cuda") for _ in range(3))
    coef = _lib.InvertCoef(0.99, 0.02)
    resid = torch.zeros(1, rows, 2, dtype=torch.float64, device="cuda")
    ws = _steps.invert_workspace(lib, rows, row_elems, "cuda")
    calls = {"plain": lambda: _steps.invert_step(lib, y, eps, out, coef=coef),
             "with_residual": lambda: _steps.invert_step(lib, y, eps, out, coef=coef, x_iter=out, resid=resid, workspace=ws)}
    res = {"n": rows * row_elems}
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


class ClockProbe:
    """Average shader clock over a stretch of stream work, as bench.py measures it: ``pf_clock_probe`` before and after, the reference
    counter's rate calibrated once against the host clock (two probes 50 ms apart)."""

    def __init__(self, lib):
        self.lib = lib
        self.buf = torch.zeros(2, 8, 2, dtype=torch.int64, device="cuda")    # [begin | end][XCD][shader cycles, reference ticks]
        self._probe(0); torch.cuda.synchronize(); t0 = time.perf_counter()
        time.sleep(0.05)
        self._probe(1); torch.cuda.synchronize(); t1 = time.perf_counter()
        b = self.buf.tolist()
        rates = sorted((b[1][x][1] - b[0][x][1]) / (t1 - t0) for x in range(8) if b[0][x][1] and b[1][x][1])
        hz = rates[len(rates) // 2] if rates else 0.0
        self.ref_hz = hz if 1e6 < hz < 1e10 else None

    def _probe(self, slot):
        _lib.check(self.lib.pf_clock_probe(self.buf[slot].data_ptr(), _lib.current_stream()), "pf_clock_probe")

    def begin(self):
        self.buf.zero_()
        self._probe(0)

    def end_mhz(self):
        self._probe(1); torch.cuda.synchronize()
        b = self.buf.tolist()
        mhz = sorted((b[1][x][0] - b[0][x][0]) / (b[1][x][1] - b[0][x][1]) * (self.ref_hz or 0) / 1e6
                     for x in range(8) if b[0][x][1] and b[1][x][1] > b[0][x][1])
        return round(mhz[len(mhz) // 2], 1) if mhz and self.ref_hz else None


def timed(fn, reps: int) -> float:
    fn()                                                   # warm-up (and the capture)
    ms = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ms)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--seed", type=int, default=1234)
    a = ap.parse_args(argv)
    _lib.require_gpu()
    p = preset("sdf_chd8bar")
    model = synthetic_model(p)
    model.ldm.eps_model.set_precision("bf16x3")
    B, t = a.batch, a.steps - 1
    cond = model._encode_chord(torch.from_numpy(synth.chords(B, 4242)).cuda())
    uc = -torch.ones(B, 1, p.d_cond, device="cuda")
    rng = np.random.default_rng(a.seed)
    x0 = torch.from_numpy((rng.random((B, p.out_channels, p.img_h, p.img_w)) > 0.97).astype(np.float32)).cuda()     # a sparse synthetic piano roll

    res = {"what": f"sdf_chd8bar synthetic weights, B={B}, {a.steps} uniform steps, K={a.iters}, {model.ldm.eps_model.precision}",
           "update_us": update_us(_lib.load(), B, p.out_channels * p.img_h * p.img_w)}
    probe = ClockProbe(_lib.load())
    res["device"] = torch.cuda.get_device_properties(0).name
    for graph in (False, True):
        s = DDIMSampler(model.ldm, a.steps, "uniform", 0.0, seed=a.seed, graph=graph)
        tag = "graph" if graph else "eager"
        probe.begin()
        res[f"ms_per_invert_step_{tag}"] = round(timed(lambda: s.invert(x0, cond, t, iters=a.iters), a.reps) / (t + 1), 3)
        res[f"sclk_mhz_invert_{tag}"] = probe.end_mhz()
        x = s.invert(x0, cond, t, iters=a.iters)
        res[f"ms_per_paint_step_{tag}"] = round(timed(lambda: s.paint(x, cond, t), a.reps) / (t + 1), 3)
    s = DDIMSampler(model.ldm, a.steps, "uniform", 0.0, seed=a.seed, graph=True)
    res["residual"] = {}
    for scale in (1.0, 5.0):
        x = s.invert(x0, cond, t, iters=a.iters, uncond_scale=scale, uncond_cond=uc)
        r = s.last_inversion.residuals()                   # [steps, iters, rows]
        back = s.paint(x, cond, t, uncond_scale=scale, uncond_cond=uc)
        res["residual"][f"scale_{scale:g}"] = {
            "last_iterate_max": float(np.nanmax(r[:, -1])), "last_iterate_median": float(np.nanmedian(r[:, -1])),
            "first_iterate_max": float(np.nanmax(r[:, 0])), "finite": bool(np.isfinite(r).all() and torch.isfinite(back).all()),
            "round_trip_max_abs": float((back - x0).abs().max()),
            "round_trip_cells_over_half_that_differ": int(((back > 0.5) != (x0 > 0.5)).sum())}
    print(json.dumps(res))
    return 0


if __name__ == "__main__":
    sys.exit(main())
