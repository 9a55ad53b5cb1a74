#!/usr/bin/env python
"""tests/golden/autoencoder.npz: the first-stage autoencoder (stable_diffusion/model/autoencoder.py of the reference) on seeded synthetic
weights (weights.synth_autoencoder_state), evaluated by the imported reference on the CPU.  Needs the reference checkout (REF of tools/make_goldens.py).

Contents (data only):
  keys / key_shapes   - the Autoencoder state_dict of the full params/autoencoder.yaml net (the training-only loss module is stubbed
                        out: it needs torchvision and holds no inference parameter)
  small_*             - channels 32, multipliers [1, 2], 1 block per level, z = emb = 4, 3 -> 3 channels; image 32x16 (latent 16x8,
                        128 attention tokens), B = 3: image, noise, mean, log_var, z = mean + std * noise, decode(z), forward with that noise
  clamp_*             - the small net with quant_conv.bias of the first / second log_var channel shifted by +20 / -30, so that log_var
                        sits at each bound of the clamp on at least 1 % of its entries: mean, log_var
  full_*              - the full net at 128x128, B = 1 (image regenerated from full_x_seed): mean, log_var, decode(mean)
"""
from __future__ import annotations

import os
import sys
import types

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from tools.make_goldens import REF, save  # noqa: E402
from polyffusion_amd.autoencoder import AutoencoderConfig  # noqa: E402
from polyffusion_amd.weights import synth_autoencoder_state  # noqa: E402

SMALL = AutoencoderConfig(in_channels=3, out_channels=3, channels=32, channel_multipliers=(1, 2), n_resnet_blocks=1, z_channels=4,
                          emb_channels=4)
FULL = AutoencoderConfig()
SMALL_HW, SMALL_B = (32, 16), 3
FULL_HW, FULL_X_SEED = (128, 128), 91
CLAMP_SHIFT = {0: 20.0, 1: -30.0}   # log_var channel -> shift of its quant_conv bias


def import_autoencoder():
    if not os.path.isdir(REF):
        raise SystemExit(f"make_goldens_autoencoder.py needs the reference at {REF}")
    # autoencoder.py imports ..losses (LPIPS + discriminator: torchvision); the loss is training code, an empty module stands in
    sys.path.insert(0, REF)
    pkg = types.ModuleType("stable_diffusion")
    pkg.__path__ = [os.path.join(REF, "stable_diffusion")]
    losses = types.ModuleType("stable_diffusion.losses")

    class LPIPSWithDiscriminator(torch.nn.Module):
        def __init__(self, **kw):
            super().__init__()

    losses.LPIPSWithDiscriminator = LPIPSWithDiscriminator
    sys.modules["stable_diffusion"], sys.modules["stable_diffusion.losses"] = pkg, losses
    import stable_diffusion.model.autoencoder as A
    return A


def ref_autoencoder(A, cfg: AutoencoderConfig, state=None):
    enc = A.Encoder(channels=cfg.channels, channel_multipliers=list(cfg.channel_multipliers), n_resnet_blocks=cfg.n_resnet_blocks,
                    in_channels=cfg.in_channels, z_channels=cfg.z_channels)
    dec = A.Decoder(channels=cfg.channels, channel_multipliers=list(cfg.channel_multipliers), n_resnet_blocks=cfg.n_resnet_blocks,
                    out_channels=cfg.out_channels, z_channels=cfg.z_channels)
    m = A.Autoencoder(enc, dec, cfg.emb_channels, cfg.z_channels)
    state = synth_autoencoder_state(cfg, 0) if state is None else state
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in state.items()}, strict=True)
    return m.eval()


def randn(seed, shape):
    return np.random.Generator(np.random.PCG64(seed)).standard_normal(shape).astype(np.float32)


class FixedNoise:
    """Stands in for the module's `torch` inside GaussianDistribution.sample: randn_like returns the recorded tensor."""
    def __init__(self, arr):
        self.arr = arr

    def randn_like(self, t):
        return torch.from_numpy(self.arr).reshape(t.shape)

    def __getattr__(self, name):
        return getattr(torch, name)


def rms(a) -> float:
    return float(np.sqrt(np.mean(np.square(np.asarray(a, dtype=np.float64)))))


def check_rms(name, a):
    r = rms(a)
    print(f"  rms({name}) = {r:.3f}")
    assert 0.1 <= r <= 30.0, f"{name}: rms {r} outside [0.1, 30] - an absolute tolerance on it would mean little"


def clamp_state(cfg: AutoencoderConfig):
    state = synth_autoencoder_state(cfg, 0)
    b = state["quant_conv.bias"].copy()
    for ch, shift in CLAMP_SHIFT.items():
        b[cfg.emb_channels + ch] += np.float32(shift)
    state["quant_conv.bias"] = b
    return state


@torch.no_grad()
def main():
    A = import_autoencoder()
    out = {}
    small = ref_autoencoder(A, SMALL)
    x = randn(11, (SMALL_B, SMALL.in_channels) + SMALL_HW)
    assert np.all(x[:, :, -1, :] != 0) and np.all(x[:, :, :, -1] != 0)   # the DownSample's padded side reads real data
    post = small.encode(torch.from_numpy(x))
    noise = randn(12, tuple(post.mean.shape))
    z = post.mean + post.std * torch.from_numpy(noise)
    out["small_x"], out["small_noise"] = x, noise
    out["small_mean"], out["small_log_var"], out["small_z"] = post.mean.numpy(), post.log_var.numpy(), z.numpy()
    out["small_dec"] = small.decode(z).numpy()
    A.torch = FixedNoise(noise)   # autoencoder.py's module-level `torch`: GaussianDistribution.sample inside forward
    try:
        fwd, _ = small(torch.from_numpy(x))
    finally:
        A.torch = torch
    out["small_forward"] = fwd.numpy()
    assert np.array_equal(out["small_forward"], out["small_dec"])
    for k in ("small_mean", "small_log_var", "small_z", "small_dec"):
        check_rms(k, out[k])

    cl = ref_autoencoder(A, SMALL, clamp_state(SMALL)).encode(torch.from_numpy(x))
    lv = cl.log_var.numpy()
    lo, hi = float(np.mean(lv == -30.0)), float(np.mean(lv == 20.0))
    print(f"  clamp: {lo:.1%} of log_var at -30, {hi:.1%} at 20")
    assert lo >= 0.01 and hi >= 0.01
    out["clamp_mean"], out["clamp_log_var"] = cl.mean.numpy(), lv

    full = ref_autoencoder(A, FULL)
    sd = full.state_dict()
    out["keys"] = np.array(list(sd))
    out["key_shapes"] = np.array([",".join(str(s) for s in v.shape) for v in sd.values()])
    xf = randn(FULL_X_SEED, (1, FULL.in_channels) + FULL_HW)
    pf = full.encode(torch.from_numpy(xf))
    out["full_x_seed"] = np.int64(FULL_X_SEED)
    out["full_mean"], out["full_log_var"] = pf.mean.numpy(), pf.log_var.numpy()
    out["full_dec"] = full.decode(pf.mean).numpy()
    for k in ("full_mean", "full_log_var", "full_dec"):
        check_rms(k, out[k])
    save("autoencoder.npz", **out)


if __name__ == "__main__":
    main()
