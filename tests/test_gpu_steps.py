"""pf_ddpm_step / pf_ddim_step (-m gpu): every route of the two entries - noise from tensors or drawn in the kernel, coefficients by value or
from a device table row named by the device step state, out of place and in place - BIT-equal to the float32 restatement of the update
(oracle.sampler_ref.ddpm_update_f32 / ddim_update_f32, itself pinned against the reference's goldens in tests/test_steps_oracle.py), and
the argument combinations the entries refuse.

Inputs are O(1) (standard normals, a 0/1 mask, the coefficient values of tests/test_gpu_round4.py), so no intermediate of the update is
subnormal and the comparison does not depend on the device's denormal mode."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import sampler_ref  # noqa: E402
from polyffusion_amd import _lib, _steps  # noqa: E402

DDPM = (1.3, 0.7, 0.2, 0.8, 0.05, 0.9, 0.43)
DDIM = (0.6, 0.8, 0.85, 0.5, 0.1, 0.8, 0.6)
OTHER = (0.3, 1.7, 0.6, 0.1, 0.9, 0.2, 1.1)          # rows 0 and 2 of the device tables: reading the wrong row changes the result
GRID = 2048 * 256                                    # threads of the largest elementwise launch: past it the grid-stride loop runs again
NMAX = 4 * GRID + 8
SEED, DQ, DP = 1234, 40, 41


@pytest.fixture(scope="module")
def lib():
    _lib.require_gpu()
    return _lib.load()


@pytest.fixture(scope="module")
def data():
    """name -> (device tensor, the same values as a numpy array) of NMAX elements; tests use the leading n (unchanged by every test)."""
    g = torch.Generator().manual_seed(7)
    host = {k: torch.randn(NMAX, generator=g) for k in ("x", "eps", "noise_p", "noise_q", "orig", "orig_noise")}
    host["mask"] = (torch.rand(NMAX, generator=g) > 0.3).float()
    return {k: (v.cuda(), v.numpy()) for k, v in host.items()}


def bits(a):
    return (a.cpu().numpy() if isinstance(a, torch.Tensor) else a).view(np.uint32)


def sources(lib, coef_cls, values, draws):
    """The two coefficient sources: host struct by value, and row 1 of a three-row device table with state = {index 1, draws}."""
    table = torch.tensor([OTHER, values, OTHER[::-1]], device="cuda")
    state = torch.zeros(2, dtype=torch.int64, device="cuda")
    _lib.check(lib.pf_step_state_set(state.data_ptr(), 1, draws, _lib.current_stream()), "pf_step_state_set")
    return dict(coef=coef_cls(*values)), dict(table=table, state=state)


def run_both_ways(step, lib, x, eps, want, **kw):
    """`step` into a fresh tensor and with x_out == x; both must equal `want` bit for bit."""
    out = step(lib, x, eps, torch.full_like(x, float("nan")), **kw)
    assert np.array_equal(bits(out), bits(want))
    xi = x.clone()
    step(lib, xi, eps, xi, **kw)
    assert np.array_equal(bits(xi), bits(want))


# ---------------------------------------------------------------------------------------------- noise from tensors
@pytest.mark.parametrize("n", [1, 5, 255, 257, GRID + 3])
def test_tensor_route_is_bit_equal_to_the_f32_oracle(lib, data, n):
    d = {k: v[0][:n] for k, v in data.items()}
    h = {k: v[1][:n] for k, v in data.items()}
    # DDPM: no noise and no known region; noise_p only; known region with both noises; known region without noise (step 0)
    for names in ((), ("noise_p",), ("noise_p", "noise_q", "orig", "mask"), ("orig", "mask")):
        want = sampler_ref.ddpm_update_f32(h["x"], h["eps"], DDPM, **{k: h[k] for k in names})
        for src in sources(lib, _lib.DdpmCoef, DDPM, 0):
            run_both_ways(_steps.ddpm_step, lib, d["x"], d["eps"], want, **src, **{k: d[k] for k in names})
    # DDIM: noise on / off x known region on / off
    for names in ((), ("noise",), ("orig", "orig_noise", "mask"), ("noise", "orig", "orig_noise", "mask")):
        want = sampler_ref.ddim_update_f32(h["x"], h["eps"], DDIM, **{k: h["noise_p" if k == "noise" else k] for k in names})
        for src in sources(lib, _lib.DdimCoef, DDIM, 0):
            run_both_ways(_steps.ddim_step, lib, d["x"], d["eps"], want, **src, **{k: d["noise_p" if k == "noise" else k] for k in names})


# ---------------------------------------------------------------------------------------------- noise drawn in the kernel
@pytest.mark.parametrize("off", [0, 4, 3 * 32768])
@pytest.mark.parametrize("n", [4, 1028, NMAX])
def test_rng_route_is_bit_equal_to_the_f32_oracle(lib, data, n, off):
    """The draws are read back with pf_randn(seed, draw, elem_offset) and handed to the oracle.  Host coefficients take the draw indices by
    value; with the device state they are (state.draws, state.draws + 1), or state.draws alone without a known region."""
    d = {k: v[0][:n] for k, v in data.items()}
    h = {k: v[1][:n] for k, v in data.items()}
    zq, zp = (_steps.randn(lib, (n,), "cuda", SEED, draw, off).cpu().numpy() for draw in (DQ, DP))
    for names in ((), ("orig", "mask")):
        want = sampler_ref.ddpm_update_f32(h["x"], h["eps"], DDPM, noise_p=zp, noise_q=zq if names else None, **{k: h[k] for k in names})
        for src in sources(lib, _lib.DdpmCoef, DDPM, DQ if names else DP):
            run_both_ways(_steps.ddpm_step, lib, d["x"], d["eps"], want, rng=(SEED, DQ, DP, off), **src, **{k: d[k] for k in names})
    for names in ((), ("orig", "orig_noise", "mask")):
        want = sampler_ref.ddim_update_f32(h["x"], h["eps"], DDIM, noise=zp, **{k: h[k] for k in names})
        for src in sources(lib, _lib.DdimCoef, DDIM, DP):
            run_both_ways(_steps.ddim_step, lib, d["x"], d["eps"], want, rng=(SEED, DP, off), **src, **{k: d[k] for k in names})


# ---------------------------------------------------------------------------------------------- refusals
def test_bad_argument_combinations_are_refused_before_any_launch(lib, data):
    base = data["x"][0]
    x, eps, other = base[:8], data["eps"][0][:8], data["orig"][0][:8]
    out = torch.zeros(8, device="cuda")
    table = torch.tensor([DDPM], device="cuda")
    state = torch.zeros(2, dtype=torch.int64, device="cuda")
    coef, icoef = _lib.DdpmCoef(*DDPM), _lib.DdimCoef(*DDIM)

    def refused(family, **fields):
        args = {"ddpm": _lib.DdpmStepArgs, "ddim": _lib.DdimStepArgs}[family]()
        kw = dict(x=x, eps=eps, x_out=out, n=8)
        kw.update(fields)
        for k, v in kw.items():
            setattr(args, k, v.data_ptr() if isinstance(v, torch.Tensor) else C.addressof(v) if isinstance(v, C.Structure) else v)
        rc = getattr(lib, f"pf_{family}_step")(C.byref(args), _lib.current_stream())
        msg = lib.pf_last_error()
        assert rc < 0 and f"{family}_step".encode() in msg, (family, fields.keys(), rc, msg)

    refused("ddpm", coef=coef, table=table, state=state)          # both coefficient sources
    refused("ddpm")                                               # neither
    refused("ddpm", table=table)                                  # a table without the state that names its row
    refused("ddpm", coef=coef, rng=1, noise_p=other)              # in-kernel draws AND a noise tensor
    refused("ddpm", coef=coef, rng=1, n=6)                        # not whole Philox groups
    refused("ddpm", coef=coef, rng=1, x=base[1:9])                # x 4 bytes off a 16-byte boundary
    refused("ddpm", coef=coef, orig=other)                        # known region without its mask
    refused("ddim", coef=icoef, orig=other, mask=other)           # DDIM known region without orig_noise
    refused("ddpm", coef=coef, x_out=None)
    refused("ddim", coef=icoef, table=table, state=state)
    refused("ddim", coef=icoef, rng=1, noise=other)
    torch.cuda.synchronize()
    assert torch.equal(out, torch.zeros(8, device="cuda"))        # nothing ran
