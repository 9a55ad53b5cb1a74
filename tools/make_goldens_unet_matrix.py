#!/usr/bin/env python
"""tests/golden/unet_matrix.npz: the real reference UNet (stable_diffusion/model/unet.py) in float32 on the CPU at three architectures
of the UNet plan matrix (tests/unet_matrix.py GOLDEN_CASES) that no other fixture holds - two transformer layers with a three-token
condition (b), transformer blocks of two widths at levels 0 and 1 on a non-square image with five tokens (c-n5), a single level with
d_cond 8 (d-16x8).  Needs the reference checkout (REF of tools/make_goldens.py); nothing of it is copied.

Contents (data only): out_<case>, the reference's eps [B, out_channels, H, W].  Weights and inputs are regenerated from their seeds
(unet_matrix.case_state / case_inputs), not stored.
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

from tools.make_goldens import import_reference, ref_unet, save  # noqa: E402
import unet_matrix as UM  # noqa: E402


@torch.no_grad()
def main():
    R = import_reference()
    out = {}
    for name in UM.GOLDEN_CASES:
        case = UM.BY_NAME[name]
        x, t, cond = UM.case_inputs(case)
        eps = ref_unet(R, case.cfg, case.seed)(torch.from_numpy(x), torch.from_numpy(t), torch.from_numpy(cond)).numpy()
        r = UM.rms(eps)
        print(f"  {name}: eps {eps.shape}, rms {r:.3f}, max |eps| {np.abs(eps).max():.3f}")
        assert eps.dtype == np.float32 and 0.1 <= r <= 30.0, f"{name}: rms {r} outside [0.1, 30] - an absolute tolerance on it would mean little"
        out["out_" + name] = eps
    save("unet_matrix.npz", **out)


if __name__ == "__main__":
    main()
