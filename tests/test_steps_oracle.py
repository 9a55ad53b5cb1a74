"""The float32 restatement of the sampler updates (oracle.sampler_ref.ddpm_update_f32 / ddim_update_f32, which the GPU tests compare
the kernels with bit for bit) pinned against the real reference's answers in tests/golden/steps.npz."""
import numpy as np

from oracle import sampler_ref
from polyffusion_amd import _lib
from polyffusion_amd.sampler import DDIMSampler, SDFSampler
from polyffusion_amd.unet import LatentDiffusion


def row(coef):
    return [getattr(coef, f) for f, _ in coef._fields_]


def test_f32_updates_vs_reference_goldens(golden):
    """Same keys and the same 2e-6 * scale tolerance as test_sampler_step_kernels_vs_reference_goldens (tests/test_gpu_ops.py); the
    coefficients are the rows the samplers build for the kernels."""
    g = golden("steps.npz")
    x, e, nz = g["x"], g["e_t"], g["noise"]
    assert x.dtype == e.dtype == nz.dtype == np.float32
    ldm = LatentDiffusion(None)
    s = SDFSampler(ldm)
    for step in (0, 1, 500, 999):
        ref = g[f"sdf_xprev_{step}"]
        got = sampler_ref.ddpm_update_f32(x, e, row(s._coef(step)), noise_p=None if step == 0 else nz)
        err = np.abs(got - ref).max()
        print(f"ddpm step {step}: max-abs-diff {err:.2e}")
        assert err <= 2e-6 * max(1.0, float(np.abs(ref).max()))
    for tag, (S, eta) in dict(u50=(50, 0.0), u20e1=(20, 1.0)).items():
        d = DDIMSampler(ldm, S, "uniform", eta)
        for idx in (0, 1, S - 1):
            ref = g[f"ddim_{tag}_xprev_{idx}"]
            got = sampler_ref.ddim_update_f32(x, e, row(d._coef(idx)), noise=nz if float(d.ddim_sigma[idx]) != 0.0 else None)
            err = np.abs(got - ref).max()
            print(f"ddim {tag} index {idx}: max-abs-diff {err:.2e}")
            assert err <= 2e-6 * max(1.0, float(np.abs(g[f"ddim_{tag}_predx0_{idx}"]).max()))


def test_step_argument_structs_match_the_header_layout():
    """pf_ddpm_step_args / pf_ddim_step_args as ctypes lays them out: the field order of include/pfhip.h, 8-byte members after `rng`."""
    assert [f for f, _ in _lib.DdpmStepArgs._fields_] == ["x", "eps", "orig", "mask", "noise_p", "noise_q", "rng", "coef", "table", "state", "seed",
                                                          "draw_q", "draw_p", "elem_offset", "x_out", "n"]
    assert [f for f, _ in _lib.DdimStepArgs._fields_] == ["x", "eps", "orig", "orig_noise", "mask", "noise", "rng", "coef", "table", "state", "seed",
                                                          "draw", "elem_offset", "x_out", "n"]
    assert _lib.DdpmStepArgs.coef.offset == 56 and _lib.DdimStepArgs.coef.offset == 56
