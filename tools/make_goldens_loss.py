#!/usr/bin/env python
"""tests/golden/loss.npz: the training objective, forward only, evaluated by the imported reference on the CPU (data only).  Build
container only; needs /root/reference.

``LatentDiffusion.loss`` (stable_diffusion/latent_diffusion.py:203-240) on the small UNet (``SMALL`` of tools/make_goldens.py) and
``DenoiseDiffusion.loss`` (ddpm/__init__.py:90-111) on the small DDPM net (``SMALL`` of tools/make_goldens_ddpm.py), synthetic weights,
B = 4.  The reference draws ``t`` with ``torch.randint`` on the global generator; the module-level ``torch`` of the two reference modules
is wrapped here so that the draw is recorded - and forced to hold 0, n_steps - 1 and a repeated value, which no seed gives at B = 4.

Contents
  sdf_* / ddpm_*   x0, cond (sdf), noise (injected), t (what the wrapped randint returned), x_t (what q_sample returned), eps_theta (what
                   the eps_model returned), loss
  gld_*            ``Polyffusion_SDF.get_loss_dict`` (models/model_sdf.py:185-234) on a chord batch, ``cond_type`` "chord" without a chord
                   encoder (the reference then flattens the chord matrix into the condition, :102-106), the same x0 / noise:
                   gld_chord [4, 8, 4]; gld_modes = cond, uncond, mix, mix; gld_seeds = the ``random.seed`` of each call;
                   gld_dropped = whether the condition became all -1; gld_t, gld_loss per call
  mix_table        rows (cond_type: 0 chord / 1 chord+txt, cond_mode: 0 mix / 1 mix2, seed, number of random.random() calls, chord part
                   all -1, texture part all -1) of get_loss_dict on a recording stand-in for ``ldm``
"""
from __future__ import annotations

import os
import random
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from tools import make_goldens as MG  # noqa: E402
from tools import make_goldens_ddpm as MD  # noqa: E402

B, N_STEPS = 4, 1000


class TorchProxy:
    """Stands in for a reference module's ``torch``: ``randint`` is recorded and forced to hold both ends and a repeat, ``randn_like``
    returns the injected noise; everything else is torch."""

    def __init__(self, noise=None):
        self.noise, self.t = noise, None

    def randint(self, low, high, size, **kw):
        t = torch.randint(low, high, size, dtype=torch.long)
        t[0], t[1], t[3] = low, high - 1, t[2]
        self.t = t.clone()
        return t

    def randn_like(self, x, **kw):
        assert self.noise is not None and tuple(self.noise.shape) == tuple(x.shape)
        return self.noise.clone()

    def __getattr__(self, name):
        return getattr(torch, name)


class CountingRandom:
    def __init__(self):
        self.calls = 0

    def random(self):
        self.calls += 1
        return random.random()


def record_loss(diff, eps_model, proxy_holder, call):
    """Run ``call()`` (a ``loss``) with the module's torch wrapped; returns (t, x_t, eps_theta, loss)."""
    seen = {}
    q0 = diff.q_sample
    diff.q_sample = lambda *a, **k: seen.setdefault("x_t", q0(*a, **k))
    hook = eps_model.register_forward_hook(lambda m, i, o: seen.__setitem__("eps_theta", o.detach().clone()))
    proxy = TorchProxy()
    proxy_holder.torch = proxy
    try:
        loss = call()
    finally:
        proxy_holder.torch = torch
        hook.remove()
        del diff.q_sample
    return proxy.t.numpy(), seen["x_t"].numpy(), seen["eps_theta"].numpy(), np.float32(loss.item())


@torch.no_grad()
def main():
    R = MG.import_reference()
    D = MD.import_ddpm()
    import stable_diffusion.latent_diffusion as ld_mod
    import models.model_sdf as sdf_mod
    torch.manual_seed(1234)
    rng = np.random.Generator(np.random.PCG64(31))
    out = {}

    ldm = MG.ref_ldm(R, MG.SMALL)
    x0 = torch.from_numpy((0.5 * rng.standard_normal((B, 2, 32, 32))).astype(np.float32))
    cond = torch.from_numpy(rng.standard_normal((B, 1, 32)).astype(np.float32))
    noise = torch.from_numpy(rng.standard_normal((B, 2, 32, 32)).astype(np.float32))
    t, xt, et, loss = record_loss(ldm, ldm.eps_model, ld_mod, lambda: ldm.loss(x0, cond, noise=noise))
    out.update(sdf_x0=x0.numpy(), sdf_cond=cond.numpy(), sdf_noise=noise.numpy(), sdf_t=t, sdf_x_t=xt, sdf_eps_theta=et, sdf_loss=loss)
    print("  sdf: t", t, "loss", loss)

    small = MD.ref_unet(D, MD.SMALL)
    diff = D.DenoiseDiffusion(small, N_STEPS)
    x0d = torch.from_numpy((0.5 * rng.standard_normal((B, 2, 32, 32))).astype(np.float32))
    noised = torch.from_numpy(rng.standard_normal((B, 2, 32, 32)).astype(np.float32))
    t, xt, et, loss = record_loss(diff, small, D, lambda: diff.loss(x0d, noise=noised))
    out.update(ddpm_x0=x0d.numpy(), ddpm_noise=noised.numpy(), ddpm_t=t, ddpm_x_t=xt, ddpm_eps_theta=et, ddpm_loss=loss)
    print("  ddpm: t", t, "loss", loss)

    # get_loss_dict on a chord batch: cond, uncond, and mix under one seed that drops the condition and one that keeps it
    chord = torch.from_numpy((rng.random((B, 8, 4)) < 0.3).astype(np.float32))
    prmat = torch.zeros(B, 128, 128)
    batch = (x0, None, chord, prmat)
    drop_seed = next(s for s in range(1000) if random.Random(s).random() < 0.2)
    keep_seed = next(s for s in range(1000) if random.Random(s).random() >= 0.2)
    modes, seeds, dropped, ts, losses = [], [], [], [], []
    for mode, seed in (("cond", 0), ("uncond", 0), ("mix", drop_seed), ("mix", keep_seed)):
        model = sdf_mod.Polyffusion_SDF(ldm, "chord", cond_mode=mode)
        seen = {}
        hook = ldm.eps_model.register_forward_hook(lambda m, i, o: seen.__setitem__("cond", i[2].detach().clone()))
        proxy = TorchProxy(noise)
        ld_mod.torch = proxy
        random.seed(seed)
        try:
            loss = model.get_loss_dict(batch, 0)["loss"]
        finally:
            ld_mod.torch = torch
            hook.remove()
        modes.append(mode); seeds.append(seed); ts.append(proxy.t.numpy()); losses.append(np.float32(loss.item()))
        dropped.append(bool((seen["cond"] == -1).all()))
        print(f"  get_loss_dict[{mode}, seed {seed}]: dropped {dropped[-1]}, loss {losses[-1]}")
    assert dropped == [False, True, True, False]
    out.update(gld_chord=chord.numpy(), gld_modes=np.array(modes), gld_seeds=np.array(seeds, np.int64), gld_dropped=np.array(dropped),
               gld_t=np.stack(ts), gld_loss=np.array(losses, np.float32))

    # the dropout choices and the number of random.random() calls, on a stand-in for ldm that records its condition
    class Recorder:
        def loss(self, x0, cond, **kw):
            self.cond = cond
            return torch.zeros(())

    rows = []
    chd, txt = torch.ones(B, 8, 4), torch.ones(B, 1, 16)
    for ct_id, ct in enumerate(("chord", "chord+txt")):
        for cm_id, cm in enumerate(("mix", "mix2")):
            for seed in range(40):
                rec, cnt = Recorder(), CountingRandom()
                model = sdf_mod.Polyffusion_SDF(rec, ct, cond_mode=cm)
                sdf_mod.random = cnt
                random.seed(seed)
                try:
                    model.get_loss_dict((x0, None, chd, txt), 0)
                finally:
                    sdf_mod.random = random
                c = rec.cond
                rows.append((ct_id, cm_id, seed, cnt.calls, int((c[..., :32] == -1).all()), int(c.shape[-1] > 32 and (c[..., 32:] == -1).all())))
    table = np.array(rows, np.int64)
    # keep, per (cond_type, cond_mode), the first seed of every distinct (chord dropped, texture dropped) outcome
    keep, seen_keys = [], set()
    for r in table:
        key = (r[0], r[1], r[4], r[5])
        if key not in seen_keys:
            seen_keys.add(key)
            keep.append(r)
    out["mix_table"] = np.array(keep, np.int64)
    print("  mix_table:\n", out["mix_table"])
    os.makedirs(MG.OUT, exist_ok=True)
    MG.save("loss.npz", **out)


if __name__ == "__main__":
    main()
