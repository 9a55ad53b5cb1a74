"""What the frames of a morph cost: the fused slerp launch against the same frames by ``pf_axpby``, and a whole morph by its parts.

    python tools/bench_morph.py [--segments 4] [--frames 5] [--steps 20] [--iters 3] [--reps 3]

prints ONE JSON line:
  * ``slerp``: per ``rows`` in {1, 16} and ``frames`` in {5, 9} at ``row_elems = 32768`` (one 2 x 128 x 128 image) - microseconds of
    ``pf_slerp_rows`` in mode slerp (two launches: reduce, combine) and in mode lerp (the combine launch alone), the bytes they move,
    ``(2 + frames) * n * 4`` (the reduce launch reads a and b once more: ``(4 + frames) * n * 4``), and GB/s; beside them the same
    frames made by ``frames`` ``pf_axpby`` launches with given weights (``3 * frames * n * 4`` bytes; the host sync and the norm launches
    that route also needs to GET its weights are not in the figure).  Each figure: the median of 5 repeats of 100 back-to-back calls
    between two events, after 20 warm-up calls, all in this one process;
  * ``morph_ms``: a full ``DDIMSampler.morph`` on sdf_chd8bar with synthetic weights - ``--segments`` rows per song, ``--frames`` frames,
    ``--steps`` uniform steps, ``--iters`` iterates, guidance 1, bf16x3 - and its three parts timed on their own: the inversion of the
    2R stacked rows, the slerp of noises and conditions, the paint of the K * R frames (wall time with a device sync around each,
    median of ``--reps`` after a warm-up call).
Nothing is asserted: the line is kept as profiles/morph_bench.json and quoted in DESIGN.md."""
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
from polyffusion_amd.sampler import DDIMSampler, morph_fractions  # noqa: E402


def event_us(call, launches: int = 100, repeats: int = 5, warmup: int = 20) -> float:
    for _ in range(warmup):
        call()
    us = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(launches):
            call()
        e1.record()
        torch.cuda.synchronize()
        us.append(e0.elapsed_time(e1) * 1e3 / launches)
    return statistics.median(us)


def slerp_us(lib, rows: int, frames: int, row_elems: int = 32768) -> dict:
    a, b = (torch.randn(rows, row_elems, device="cuda") for _ in range(2))
    fr = morph_fractions(frames)
    out = torch.empty(frames, rows, row_elems, device="cuda")
    ws = _steps.slerp_workspace(lib, rows, row_elems, "cuda")
    n = rows * row_elems
    w = [(float(np.float32(1 - t)), float(np.float32(t))) for t in fr]

    def by_axpby():
        for k in range(frames):
            _lib.check(lib.pf_axpby(a.data_ptr(), b.data_ptr(), w[k][0], w[k][1], out[k].data_ptr(), n, _lib.current_stream()), "pf_axpby", lib)

    res = {"rows": rows, "frames": frames, "n": n}
    for name, call, nbytes in (("slerp", lambda: _steps.slerp_rows(lib, a, b, fr, out=out, want_stats=False, workspace=ws), (4 + frames) * n * 4),
                               ("lerp", lambda: _steps.slerp_rows(lib, a, b, fr, mode="lerp", out=out, want_stats=False), (2 + frames) * n * 4),
                               ("axpby", by_axpby, 3 * frames * n * 4)):
        us = event_us(call)
        res[name] = {"us": round(us, 2), "bytes": nbytes, "gb_per_s": round(nbytes / us / 1e3, 1)}
    return res


def timed(fn, reps: int) -> float:
    fn()                                                   # warm-up
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
    ap.add_argument("--segments", type=int, default=4)
    ap.add_argument("--frames", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--seed", type=int, default=1234)
    a = ap.parse_args(argv)
    _lib.require_gpu()
    lib = _lib.load()
    res = {"device": torch.cuda.get_device_properties(0).name,
           "slerp": [slerp_us(lib, rows, frames) for rows in (1, 16) for frames in (5, 9)]}
    p = preset("sdf_chd8bar")
    model = synthetic_model(p)
    model.ldm.eps_model.set_precision("bf16x3")
    R, K, t = a.segments, a.frames, a.steps - 1
    ca, cb = (model._encode_chord(torch.from_numpy(synth.chords(R, seed)).cuda()) for seed in (4242, 4343))
    rng = np.random.default_rng(a.seed)
    xa, xb = (torch.from_numpy((rng.random((R, p.out_channels, p.img_h, p.img_w)) > 0.97).astype(np.float32)).cuda() for _ in range(2))
    s = DDIMSampler(model.ldm, a.steps, "uniform", 0.0, seed=a.seed)
    fr = morph_fractions(K)
    x = s.invert(torch.cat([xa, xb]), torch.cat([ca, cb]), t, iters=a.iters)
    xs = s.morph_noise(x[:R], x[R:], fr)[0]
    cs = s.morph_cond(ca, cb, fr)
    res["what"] = f"sdf_chd8bar synthetic weights, {R} segments per song, {K} frames, {a.steps} uniform steps, K={a.iters}, {model.ldm.eps_model.precision}"
    res["morph_ms"] = {
        "whole": round(timed(lambda: s.morph(xa, ca, xb, cb, K, t_end=t, iters=a.iters), a.reps), 2),
        "inversion": round(timed(lambda: s.invert(torch.cat([xa, xb]), torch.cat([ca, cb]), t, iters=a.iters), a.reps), 2),
        "slerp": round(timed(lambda: (s.morph_noise(x[:R], x[R:], fr), s.morph_cond(ca, cb, fr)), a.reps), 3),
        "paint": round(timed(lambda: s._morph_paint(xs, cs, t, 16, 1.0, None, None), a.reps), 2)}
    print(json.dumps(res))
    return 0


if __name__ == "__main__":
    sys.exit(main())
