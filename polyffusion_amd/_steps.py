"""The sampler's elementwise launches: noise, ``a*x + b*y`` and the two reverse-step updates (``pf_randn`` / ``pf_randn_dev``, ``pf_axpby``,
``pf_ddpm_step``, ``pf_ddim_step`` of include/pfhip.h).  The only place that fills ``pf_ddpm_step_args`` / ``pf_ddim_step_args``:
``sampler.py`` and ``ddpm.py`` decide WHICH route a step takes (coefficients by value or from a device table, noise tensors or
in-kernel draws) and say so with keyword arguments; every launch goes to the current stream.  Tensors are read as dense buffers
through raw pointers: callers pass contiguous float32 tensors.

``owner`` (``draw`` / ``q_sample``): a sampler object with ``_lib``, ``noise_fn``, ``seed`` and the draw counter ``_draws``."""
from __future__ import annotations

import ctypes as C

import torch

from . import _lib


def randn(lib, shape, device, seed, draw, elem_offset) -> torch.Tensor:
    """Draw ``draw`` of the counter-based generator; ``elem_offset`` = index of the first element in the unsharded tensor."""
    out = torch.empty(tuple(shape), dtype=torch.float32, device=device)
    _lib.check(lib.pf_randn(out.data_ptr(), out.numel(), int(seed), int(draw), int(elem_offset), _lib.current_stream()), "pf_randn", lib)
    return out


def randn_dev(lib, out, seed, state, slot, elem_offset) -> torch.Tensor:
    """``randn`` into ``out`` with the draw index read on the device: ``state.draws + slot`` (captured steps)."""
    _lib.check(lib.pf_randn_dev(out.data_ptr(), out.numel(), int(seed), state.data_ptr(), int(slot), int(elem_offset), _lib.current_stream()),
               "pf_randn_dev", lib)
    return out


def draw(owner, shape, device, elem_offset=0) -> torch.Tensor:
    """The owner's next noise tensor: ``noise_fn(shape)`` when it has one (an injected tape), else the next draw of its seed."""
    if owner.noise_fn is not None:
        return owner.noise_fn(tuple(shape)).to(device=device, dtype=torch.float32).contiguous()
    out = randn(owner._lib, shape, device, owner.seed, owner._draws, elem_offset)
    owner._draws += 1
    return out


def axpby(lib, x, y, a, b) -> torch.Tensor:
    x, y = x.contiguous(), y.contiguous()
    out = torch.empty_like(x)
    _lib.check(lib.pf_axpby(x.data_ptr(), y.data_ptr(), float(a), float(b), out.data_ptr(), out.numel(), _lib.current_stream()), "pf_axpby", lib)
    return out


def q_sample(owner, x0, noise, a, b, elem_offset=0) -> torch.Tensor:
    """``a * x0 + b * noise``, the noise drawn from the owner when not given."""
    if noise is None:
        noise = draw(owner, x0.shape, x0.device, elem_offset)
    return axpby(owner._lib, x0, noise, a, b)


def _launch(fn, what, lib, args, x, eps, out, coef, table, state, rng, rng_fields, tensors):
    for k, v in tensors.items():
        setattr(args, k, _lib.ptr(v))
    args.x, args.eps, args.x_out, args.n = x.data_ptr(), eps.data_ptr(), out.data_ptr(), x.numel()
    args.coef = None if coef is None else C.addressof(coef)     # copied by the library during the call
    args.table, args.state = _lib.ptr(table), _lib.ptr(state)
    if rng is not None:
        args.rng = 1
        for k, v in zip(rng_fields, rng):
            setattr(args, k, int(v))
    _lib.check(fn(C.byref(args), _lib.current_stream()), what, lib)
    return out


def ddpm_step(lib, x, eps, out, *, coef=None, table=None, state=None, noise_p=None, noise_q=None, rng=None, orig=None, mask=None):
    """One DDPM / RePaint update into ``out`` (may be ``x``).  ``coef`` (a host ``DdpmCoef``) or ``table`` + ``state`` (device);
    ``rng``: ``None`` (noise from ``noise_p`` / ``noise_q``, ``None`` = no such term) or ``(seed, draw_q, draw_p, elem_offset)``."""
    return _launch(lib.pf_ddpm_step, "pf_ddpm_step", lib, _lib.DdpmStepArgs(), x, eps, out, coef, table, state, rng,
                   ("seed", "draw_q", "draw_p", "elem_offset"), dict(noise_p=noise_p, noise_q=noise_q, orig=orig, mask=mask))


def ddim_step(lib, x, eps, out, *, coef=None, table=None, state=None, noise=None, rng=None, orig=None, orig_noise=None, mask=None):
    """One DDIM update into ``out`` (may be ``x``).  ``rng``: ``None`` (noise from ``noise``) or ``(seed, draw, elem_offset)``."""
    return _launch(lib.pf_ddim_step, "pf_ddim_step", lib, _lib.DdimStepArgs(), x, eps, out, coef, table, state, rng,
                   ("seed", "draw", "elem_offset"), dict(noise=noise, orig=orig, orig_noise=orig_noise, mask=mask))
