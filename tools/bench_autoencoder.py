#!/usr/bin/env python
"""Throughput of the first-stage autoencoder (pf_autoenc: encode = image -> posterior moments + sample, decode = latent -> image) at
full size (params/autoencoder.yaml, 128x128, seeded synthetic weights).  One JSON line: per precision (the default split mode and f32)
ms per encode and per decode at B = 16, launches, FLOPs and the achieved TFLOP/s.  Timing as tools/bench_ddpm.py: HIP events around
`--steps` calls, `--windows` windows after `--warmup` calls, the median window reported."""
from __future__ import annotations

import argparse
import json
import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from bench import _median  # noqa: E402
from polyffusion_amd import _lib  # noqa: E402
from polyffusion_amd.autoencoder import Autoencoder, AutoencoderConfig  # noqa: E402
from polyffusion_amd.weights import synth_autoencoder_state  # noqa: E402


def _time(fn, steps, warmup, windows):
    for _ in range(warmup):
        out = fn()
    secs = []
    for _ in range(max(1, windows)):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(steps):
            out = fn()
        e1.record()
        torch.cuda.synchronize()
        secs.append(e0.elapsed_time(e1) * 1e-3 / steps)
    assert torch.isfinite(out).all().item(), "non-finite output"
    return _median(secs), secs


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--size", type=int, default=128)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--windows", type=int, default=3)
    ap.add_argument("--x3", choices=("bf16", "f16"), default="bf16", help="element type of the split mode (which library build)")
    args = ap.parse_args(argv)
    _lib.require_gpu()
    cfg = AutoencoderConfig()
    ae = Autoencoder(cfg, x3="f16" if args.x3 == "f16" else None)
    ae.load_state_dict(synth_autoencoder_state(cfg, 0))
    B, S, zs = args.batch, args.size, args.size // cfg.downscale
    x = torch.empty(B, cfg.in_channels, S, S, device=ae.device)
    _lib.check(ae._lib.pf_randn(x.data_ptr(), x.numel(), 0, 0, 0, _lib.current_stream()), "pf_randn", ae._lib)
    res = {"workload": "autoencoder", "batch": B, "image": [S, S], "latent": [cfg.emb_channels, zs, zs]}
    for mode in (ae._split_name, "f32"):
        ae.set_precision(mode)
        z = ae.encode_sample(x, seed=1)[0]
        enc, enc_w = _time(lambda: ae.encode_sample(x, seed=1)[0], args.steps, args.warmup, args.windows)
        dec, dec_w = _time(lambda: ae.decode(z), args.steps, args.warmup, args.windows)
        ef, df = ae.encode_flops(B, S, S), ae.decode_flops(B, zs, zs)
        res[mode] = {
            "encode_ms": round(enc * 1e3, 3), "decode_ms": round(dec * 1e3, 3),
            "encode_window_ms": [round(v * 1e3, 3) for v in enc_w], "decode_window_ms": [round(v * 1e3, 3) for v in dec_w],
            "encode_launches": ae.encode_launches(B, S, S), "decode_launches": ae.decode_launches(B, zs, zs),
            "encode_flops": ef, "decode_flops": df,
            "encode_tflops": round(ef / enc / 1e12, 2), "decode_tflops": round(df / dec / 1e12, 2),
        }
    print(json.dumps(res))


if __name__ == "__main__":
    main()
