"""The sampler's elementwise launches: noise, ``a*x + b*y`` and the three reverse-step updates (``pf_randn`` / ``pf_randn_dev``, ``pf_axpby``,
``pf_ddpm_step``, ``pf_ddim_step``, ``pf_dpm_step``, ``pf_dpm_sde_step`` of include/pfhip.h), the upward iterate of exact DDIM inversion (``pf_invert_step``),
the frames between two tensors of a morph (``pf_slerp_rows``), the guidance combine rescaled per row (``pf_cfg_rescale``),
eps rewritten so that its predicted x0 is clipped or dynamically thresholded (``pf_x0_threshold``),
the two launches around the denoiser of a window plan
(``pf_window_split``, ``pf_window_merge``), and the two launches of the training objective (``pf_qsample_rows``,
``pf_mse_rows``) with the loss evaluation both diffusion mirrors share (``diffusion_loss_rows``).  The only place that fills
``pf_ddpm_step_args`` / ``pf_ddim_step_args`` / ``pf_dpm_step_args`` / ``pf_qsample_rows_args`` / ``pf_mse_rows_args``:
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


def dpm_step(lib, x, eps, out, *, coef=None, table=None, state=None, x0_prev=None, x0_out=None, orig=None, orig_noise=None, mask=None):
    """One DPM-Solver++(2M) update into ``out`` (may be ``x``).  ``x0_prev``: the previous step's data prediction, read only by a
    second-order step (``c_1 != 0``); ``x0_out``: receives this step's (may be ``x0_prev``; ``None`` = not kept).  No noise is drawn."""
    return _launch(lib.pf_dpm_step, "pf_dpm_step", lib, _lib.DpmStepArgs(), x, eps, out, coef, table, state, None, (),
                   dict(x0_prev=x0_prev, x0_out=x0_out, orig=orig, orig_noise=orig_noise, mask=mask))


def dpm_sde_step(lib, x, eps, out, *, coef=None, table=None, state=None, x0_prev=None, x0_out=None, noise=None, rng=None, orig=None,
                 orig_noise=None, mask=None):
    """One update of the stochastic DPM-Solver++(2M) into ``out`` (may be ``x``): ``dpm_step`` with ``sigma_n * z`` added before the
    known-region blend.  ``coef``: a host ``DpmSdeCoef``, or ``table`` (rows of 8 floats) + ``state``.  ``rng``: ``None`` (z from ``noise``,
    read only when ``sigma_n != 0``) or ``(seed, draw, elem_offset)`` (drawn in the kernel; ``draw`` comes from ``state`` when that is set)."""
    return _launch(lib.pf_dpm_sde_step, "pf_dpm_sde_step", lib, _lib.DpmSdeStepArgs(), x, eps, out, coef, table, state, rng,
                   ("seed", "draw", "elem_offset"), dict(x0_prev=x0_prev, x0_out=x0_out, noise=noise, orig=orig, orig_noise=orig_noise, mask=mask))


def invert_workspace(lib, rows: int, row_elems: int, device) -> torch.Tensor:
    """The float64 workspace ``invert_step`` needs for the residual of ``rows`` rows of ``row_elems`` floats."""
    nb = int(lib.pf_invert_step_workspace_bytes(int(rows), int(row_elems)))
    return torch.empty(max(nb, 8) // 8, dtype=torch.float64, device=device)


def invert_step(lib, y, eps, out, *, coef=None, table=None, state=None, x_iter=None, resid=None, workspace=None, iters: int = 1, k: int = 0,
                slot: int = 0):
    """One fixed-point iterate of one upward DDIM step into ``out`` (``pf_invert_step``): ``out = c_y*y + c_e*eps`` on ``[rows, ...]`` tensors,
    rows = ``y.shape[0]``.  ``out`` may be ``x_iter``, never ``y``.  ``coef`` (a host ``InvertCoef``) or ``table`` + ``state`` (device).
    ``resid``: float64 ``[..., rows, 2]`` on the device, its leading dimensions the slots - the launch then also writes the row sums of
    ``(out - x_iter) ** 2`` (``x_iter = None``: ``y``) and ``out ** 2`` into slot ``state.index * iters + k`` (with ``state``) or ``slot``;
    it needs ``workspace`` (``invert_workspace``)."""
    a = _lib.InvertStepArgs()
    rows = int(y.shape[0])
    a.y, a.eps, a.x_iter, a.x_out = y.data_ptr(), eps.data_ptr(), _lib.ptr(x_iter), out.data_ptr()
    a.coef = None if coef is None else C.addressof(coef)        # copied by the library during the call
    a.table, a.state = _lib.ptr(table), _lib.ptr(state)
    a.rows, a.row_elems = rows, y.numel() // max(1, rows)
    if resid is not None:
        a.resid, a.n_slots = resid.data_ptr(), resid.numel() // (2 * rows)
        a.workspace, a.workspace_bytes = _lib.ptr(workspace), 0 if workspace is None else workspace.numel() * workspace.element_size()
        a.iters, a.k, a.slot = int(iters), int(k), int(slot)
    _lib.check(lib.pf_invert_step(C.byref(a), _lib.current_stream()), "pf_invert_step", lib)
    return out


def slerp_workspace(lib, rows: int, row_elems: int, device) -> torch.Tensor:
    """The float64 workspace mode slerp of ``slerp_rows`` needs for ``rows`` rows of ``row_elems`` floats."""
    nb = int(lib.pf_slerp_rows_workspace_bytes(int(rows), int(row_elems)))
    return torch.empty(max(nb, 8) // 8, dtype=torch.float64, device=device)


def slerp_rows(lib, a, b, fracs, *, mode: str = "slerp", out=None, want_stats: bool = True, workspace=None):
    """``len(fracs)`` points between the rows of ``a`` and ``b`` (``pf_slerp_rows``): ``out[k] = w0[k]*a + w1[k]*b`` with one weight pair per
    (frame, row), rows = ``a.shape[0]`` - on the great circle through the two rows (``mode="slerp"``: a reduce and a combine launch) or on
    the chord (``"lerp"``: the combine launch alone).  ``fracs``: host floats in [0, 1]; 0 and 1 give copies of ``a`` and ``b``.  ``a`` and
    ``b`` are made contiguous float32.  Returns ``(out [K, rows, ...], stats, weights)``: ``stats`` float64 ``[rows, 3]`` (the sums a*a, a*b,
    b*b; slerp only) and ``weights`` float32 ``[K, rows, 2]`` on the device, both ``None`` without ``want_stats``.  No host sync."""
    a, b = a.contiguous().float(), b.contiguous().float()
    if a.shape != b.shape or a.dim() < 1:
        raise ValueError(f"slerp_rows: endpoints of shapes {tuple(a.shape)} and {tuple(b.shape)}")
    if mode not in _lib.SLERP_MODES:
        raise ValueError(f"slerp_rows: mode {mode!r}, expected one of {tuple(_lib.SLERP_MODES)}")
    fr = [float(v) for v in fracs]
    K, rows = len(fr), int(a.shape[0])
    row_elems = a.numel() // max(1, rows)
    if out is None:
        out = torch.empty((K,) + tuple(a.shape), dtype=torch.float32, device=a.device)
    elif out.dtype != torch.float32 or not out.is_contiguous() or out.numel() != K * a.numel():
        raise ValueError(f"slerp_rows: out must be contiguous float32 of {K} x {tuple(a.shape)}")
    stats = weights = None
    if want_stats:
        stats = torch.zeros(rows, 3, dtype=torch.float64, device=a.device) if mode == "slerp" else None
        weights = torch.empty(K, rows, 2, dtype=torch.float32, device=a.device)
    args = _lib.SlerpArgs()
    tarr = (C.c_double * max(1, K))(*fr)                            # copied by the library during the call
    args.a, args.b, args.t, args.out = a.data_ptr(), b.data_ptr(), C.addressof(tarr), out.data_ptr()
    args.stats, args.weights = _lib.ptr(stats), _lib.ptr(weights)
    args.mode, args.frames, args.rows, args.row_elems = _lib.SLERP_MODES[mode], K, rows, row_elems
    if mode == "slerp":
        if workspace is None and rows > 0:
            workspace = slerp_workspace(lib, rows, row_elems, a.device)
        args.workspace, args.workspace_bytes = _lib.ptr(workspace), 0 if workspace is None else workspace.numel() * workspace.element_size()
    _lib.check(lib.pf_slerp_rows(C.byref(args), _lib.current_stream()), "pf_slerp_rows", lib)
    return out, stats, weights


def cfg_rescale_workspace(lib, rows: int, row_elems: int, device) -> torch.Tensor:
    """The float64 workspace ``cfg_rescale`` needs for ``rows`` rows of ``row_elems`` floats."""
    nb = int(lib.pf_cfg_rescale_workspace_bytes(int(rows), int(row_elems)))
    return torch.empty(max(nb, 8) // 8, dtype=torch.float64, device=device)


def cfg_rescale(lib, epsg, groups: int, scales, phi: float, *, out=None, want_stats: bool = False, workspace=None):
    """The guidance combine of ``epsg`` ``[groups * rows, ...]`` (group-major, as the guided evaluation stacks it; ``groups`` 2 or 3, ``scales``
    ``(s,)`` or ``(s1, s2)`` as ``guidance_plan`` returns them), every row scaled by ``w = phi * f + (1 - phi)`` with ``f`` the ratio of the
    per-row standard deviations of the conditional group and of the combine (``pf_cfg_rescale``: a reduce and a combine launch; a row is
    one batch entry).  Returns ``(out [rows, ...], stats, weights)``: ``stats`` float64 ``[rows, 3]`` (``var_pos``, ``var_cfg``, ``f``) and
    ``weights`` float32 ``[rows]`` on the device, both ``None`` without ``want_stats``.  No host sync."""
    groups = int(groups)
    if epsg.dtype != torch.float32 or not epsg.is_contiguous():
        raise ValueError("cfg_rescale: epsg must be contiguous float32")
    if groups < 1 or epsg.dim() < 1 or epsg.shape[0] % groups != 0:
        raise ValueError(f"cfg_rescale: epsg of shape {tuple(epsg.shape)} is not {groups} groups of rows")
    rows = epsg.shape[0] // groups
    shape = (rows,) + tuple(epsg.shape[1:])
    row_elems = epsg.numel() // max(1, groups * rows)
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=epsg.device)
    elif out.dtype != torch.float32 or not out.is_contiguous() or out.numel() != rows * row_elems:
        raise ValueError(f"cfg_rescale: out must be contiguous float32 of {shape}")
    stats = weights = None
    if want_stats:
        stats = torch.empty(rows, 3, dtype=torch.float64, device=epsg.device)
        weights = torch.empty(rows, dtype=torch.float32, device=epsg.device)
    if workspace is None and rows > 0:
        workspace = cfg_rescale_workspace(lib, rows, row_elems, epsg.device)
    a = _lib.CfgRescaleArgs()
    a.epsg, a.eps, a.stats, a.weights = epsg.data_ptr(), out.data_ptr(), _lib.ptr(stats), _lib.ptr(weights)
    a.workspace, a.workspace_bytes = _lib.ptr(workspace), 0 if workspace is None else workspace.numel() * workspace.element_size()
    a.phi = float(phi)
    a.s1, a.s2 = (float(v) for v in (tuple(scales) + (0.0, 0.0))[:2])
    a.groups, a.rows, a.row_elems = groups, rows, row_elems
    _lib.check(lib.pf_cfg_rescale(C.byref(a), _lib.current_stream()), "pf_cfg_rescale", lib)
    return out, stats, weights


def x0_threshold_table(alpha_bar) -> torch.Tensor:
    """The coefficient table of ``pf_x0_threshold`` on the host, float32 ``[n_steps, 4]``: ``1/sqrt(ab)``, ``sqrt(1-ab)/sqrt(ab)``,
    ``1/sqrt(1-ab)``, ``sqrt(ab)/sqrt(1-ab)`` of the model's float32 ``alpha_bar``, computed in float64 and rounded once."""
    ab = alpha_bar.detach().to(device="cpu", dtype=torch.float32).double()
    ra, rb = torch.sqrt(ab), torch.sqrt(1.0 - ab)
    return torch.stack([1.0 / ra, rb / ra, 1.0 / rb, ra / rb], dim=1).float().contiguous()


_X0T_WORKSPACES = {}      # str(device) -> the largest workspace x0_threshold has needed there


def x0_threshold_workspace(lib, rows: int, row_elems: int, device, form: str = "auto"):
    """The workspace ``x0_threshold`` needs (``None``: none - the resident form), cached per device and grown on demand.  While a stream
    is being captured nothing is cached: a buffer allocated there belongs to the graph's pool."""
    nb = int(lib.pf_x0_threshold_workspace_bytes(int(rows), int(row_elems), _lib.X0T_FORMS[form]))
    if nb == 0:
        return None
    key = str(device)
    ws = _X0T_WORKSPACES.get(key)
    if ws is None or ws.numel() * 8 < nb:
        ws = torch.empty((nb + 7) // 8, dtype=torch.int64, device=device)
        if not (device.type == "cuda" and torch.cuda.is_current_stream_capturing()):
            _X0T_WORKSPACES[key] = ws
    return ws


def x0_threshold(lib, x, eps, t, table, *, mode: str = "dynamic", p: float = 0.995, range=(0.0, 1.0), s_max: float = float("inf"),
                 t_stride: int = 1, out=None, want_stats: bool = False, form: str = "auto", workspace=None):
    """``eps`` ``[rows, ...]`` rewritten so that the x0 it predicts from ``x`` is clipped to ``range`` (``mode="clip"``) or dynamically
    thresholded at the ``p``-quantile of its own magnitudes (``mode="dynamic"``; ``pf_x0_threshold``).  ``x`` ``[rows, ...]`` may have more
    elements per row than ``eps`` (``cond_concat`` channels behind the first ones); row ``r`` reads its time-step value at
    ``t[r * t_stride]`` (device int64) and its coefficients in ``table`` (``x0_threshold_table`` on the device).  ``out``: ``None`` (a new
    tensor), ``eps`` itself (in place) or a disjoint tensor.  Returns ``(out, stats)``: ``stats`` float64 ``[rows, 4]`` on the device
    (``q``, ``s``, ``w``, changed elements), ``None`` without ``want_stats``.  No host sync."""
    if mode not in _lib.X0T_MODES:
        raise ValueError(f"x0_threshold: mode {mode!r}, expected one of {sorted(_lib.X0T_MODES)}")
    if form not in _lib.X0T_FORMS:
        raise ValueError(f"x0_threshold: form {form!r}, expected one of {sorted(_lib.X0T_FORMS)}")
    for name, v in (("x", x), ("eps", eps)):
        if v.dtype != torch.float32 or not v.is_contiguous():
            raise ValueError(f"x0_threshold: {name} must be contiguous float32")
    if t.dtype != torch.int64 or not t.is_contiguous() or table.dtype != torch.float32 or not table.is_contiguous() or table.dim() != 2 or table.shape[1] != 4:
        raise ValueError("x0_threshold: t must be contiguous int64 and table contiguous float32 [n, 4]")
    rows = eps.shape[0] if eps.dim() else 0
    if rows == 0 or x.dim() == 0 or x.shape[0] != rows:
        raise ValueError(f"x0_threshold: x of shape {tuple(x.shape)} and eps of shape {tuple(eps.shape)} do not have the same rows")
    row_elems, x_stride = eps.numel() // rows, x.numel() // rows
    if t.numel() < (rows - 1) * int(t_stride) + 1:
        raise ValueError(f"x0_threshold: t of {t.numel()} entries for {rows} rows at stride {t_stride}")
    if out is None:
        out = torch.empty_like(eps)
    elif out.dtype != torch.float32 or not out.is_contiguous() or out.shape != eps.shape:
        raise ValueError(f"x0_threshold: out must be contiguous float32 of {tuple(eps.shape)}")
    stats = torch.empty(rows, 4, dtype=torch.float64, device=eps.device) if want_stats else None
    if workspace is None:
        workspace = x0_threshold_workspace(lib, rows, row_elems, eps.device, form)
    a = _lib.X0ThresholdArgs()
    a.x, a.x_row_stride, a.eps, a.eps_out = x.data_ptr(), x_stride, eps.data_ptr(), out.data_ptr()
    a.t, a.t_stride, a.table, a.n_table = t.data_ptr(), int(t_stride), table.data_ptr(), table.shape[0]
    a.stats, a.workspace = _lib.ptr(stats), _lib.ptr(workspace)
    a.workspace_bytes = 0 if workspace is None else workspace.numel() * workspace.element_size()
    a.p, a.s_max, (a.lo, a.hi) = float(p), float(s_max), (float(range[0]), float(range[1]))
    a.mode, a.form, a.rows, a.row_elems = _lib.X0T_MODES[mode], _lib.X0T_FORMS[form], rows, row_elems
    _lib.check(lib.pf_x0_threshold(C.byref(a), _lib.current_stream()), "pf_x0_threshold", lib)
    return out, stats


def x0_predict(lib, x, eps, t, table, *, t_stride: int = 1, out=None) -> torch.Tensor:
    """The predicted clean image of every row of ``eps`` ``[rows, ...]`` (``pf_x0_predict``): the expression ``x0_threshold`` bounds, written
    out.  ``x``, ``t``, ``table`` and ``t_stride`` as there; ``out``: ``None`` (a new tensor) or a tensor disjoint from the inputs.  No host sync."""
    for name, v in (("x", x), ("eps", eps)):
        if v.dtype != torch.float32 or not v.is_contiguous():
            raise ValueError(f"x0_predict: {name} must be contiguous float32")
    if t.dtype != torch.int64 or not t.is_contiguous() or table.dtype != torch.float32 or not table.is_contiguous() or table.dim() != 2 or table.shape[1] != 4:
        raise ValueError("x0_predict: t must be contiguous int64 and table contiguous float32 [n, 4]")
    rows = eps.shape[0] if eps.dim() else 0
    if rows == 0 or x.dim() == 0 or x.shape[0] != rows:
        raise ValueError(f"x0_predict: x of shape {tuple(x.shape)} and eps of shape {tuple(eps.shape)} do not have the same rows")
    if t.numel() < (rows - 1) * int(t_stride) + 1:
        raise ValueError(f"x0_predict: t of {t.numel()} entries for {rows} rows at stride {t_stride}")
    if out is None:
        out = torch.empty_like(eps)
    elif out.dtype != torch.float32 or not out.is_contiguous() or out.shape != eps.shape:
        raise ValueError(f"x0_predict: out must be contiguous float32 of {tuple(eps.shape)}")
    a = _lib.X0PredictArgs()
    a.x, a.x_row_stride, a.eps = x.data_ptr(), x.numel() // rows, eps.data_ptr()
    a.t, a.t_stride, a.table, a.n_table = t.data_ptr(), int(t_stride), table.data_ptr(), table.shape[0]
    a.x0, a.rows, a.row_elems = out.data_ptr(), rows, eps.numel() // rows
    _lib.check(lib.pf_x0_predict(C.byref(a), _lib.current_stream()), "pf_x0_predict", lib)
    return out


def steer_resample(lib, reward, base, n: int, *, lam: float, ess: float, seed: int, group_offset: int, event: int):
    """One resampling decision per group of ``n`` consecutive particles (``pf_steer_resample``): ``reward`` / ``base`` float64
    ``[groups * n]`` on the device, ``base`` updated in place where a group resamples.  Returns ``(ancestors int32 [groups * n]
    group-local, weights float64 [groups * n], stats float64 [groups, 4] = ESS, sum of weights, flag, u)``, all on the device.  No host sync."""
    for name, v in (("reward", reward), ("base", base)):
        if v.dtype != torch.float64 or not v.is_contiguous() or v.dim() != 1:
            raise ValueError(f"steer_resample: {name} must be a contiguous float64 vector")
    n = int(n)
    if n < 1 or reward.numel() == 0 or reward.numel() % n != 0 or base.numel() != reward.numel():
        raise ValueError(f"steer_resample: {reward.numel()} rewards and {base.numel()} base values are not whole groups of {n}")
    groups, dev = reward.numel() // n, reward.device
    anc = torch.empty(groups * n, dtype=torch.int32, device=dev)
    weights = torch.empty(groups * n, dtype=torch.float64, device=dev)
    stats = torch.empty(groups, 4, dtype=torch.float64, device=dev)
    a = _lib.SteerResampleArgs(reward=reward.data_ptr(), base=base.data_ptr(), lam=float(lam), ess_frac=float(ess), seed=int(seed) & (2 ** 64 - 1),
                               group_offset=int(group_offset), event=int(event), ancestors=anc.data_ptr(), weights=weights.data_ptr(),
                               stats=stats.data_ptr(), groups=groups, n=n)
    _lib.check(lib.pf_steer_resample(C.byref(a), _lib.current_stream()), "pf_steer_resample", lib)
    return anc, weights, stats


def rows_gather(lib, srcs, ancestors, n: int, per: int = 1, outs=None) -> list:
    """Every tensor of ``srcs`` (up to four, float32 ``[groups * n * per, ...]``) with the rows of particle ``j`` of a group replaced by those
    of particle ``ancestors[j]`` of the same group, in ONE launch (``pf_rows_gather``).  ``outs``: ``None`` (new tensors) or tensors disjoint
    from every source.  Returns the list of results.  No host sync."""
    srcs = list(srcs)
    if not 1 <= len(srcs) <= _lib.GATHER_MAX_TENSORS:
        raise ValueError(f"rows_gather: {len(srcs)} tensors, expected 1 to {_lib.GATHER_MAX_TENSORS}")
    n, per = int(n), int(per)
    if ancestors.dtype != torch.int32 or not ancestors.is_contiguous() or n < 1 or per < 1 or ancestors.numel() == 0 or ancestors.numel() % n != 0:
        raise ValueError(f"rows_gather: ancestors must be contiguous int32, whole groups of {n}")
    groups = ancestors.numel() // n
    rows = groups * n * per
    outs = [torch.empty_like(v) for v in srcs] if outs is None else list(outs)
    a = _lib.RowsGatherArgs()
    for k, (v, o) in enumerate(zip(srcs, outs)):
        if v.dtype != torch.float32 or not v.is_contiguous() or v.dim() == 0 or v.shape[0] != rows:
            raise ValueError(f"rows_gather: tensor {k} of shape {tuple(v.shape)} is not contiguous float32 with {rows} rows ({groups} groups of {n} x {per})")
        if o.dtype != torch.float32 or not o.is_contiguous() or o.shape != v.shape:
            raise ValueError(f"rows_gather: out {k} must be contiguous float32 of {tuple(v.shape)}")
        a.src[k], a.dst[k], a.row_elems[k] = v.data_ptr(), o.data_ptr(), v.numel() // rows
    a.n_tensors, a.ancestors, a.groups, a.n, a.per = len(srcs), ancestors.data_ptr(), groups, n, per
    _lib.check(lib.pf_rows_gather(C.byref(a), _lib.current_stream()), "pf_rows_gather", lib)
    return outs


def window_split(lib, canvas, n_windows: int, stride: int, win_h: int) -> torch.Tensor:
    """Canvas ``[S, C, canvas_h, W]`` -> its windows ``[S * n_windows, C, win_h, W]``, song-major (``pf_window_split``)."""
    S, ch, _, W = canvas.shape
    out = torch.empty(S * n_windows, ch, win_h, W, dtype=torch.float32, device=canvas.device)
    _lib.check(lib.pf_window_split(canvas.data_ptr(), out.data_ptr(), S, ch, win_h, W, n_windows, stride, _lib.current_stream()),
               "pf_window_split", lib)
    return out


def window_merge(lib, eps, row_weight, songs: int, n_windows: int, stride: int, groups: int = 1, scales=(), out=None) -> torch.Tensor:
    """The windows' eps ``[groups * S * n_windows, C, win_h, W]`` (group-major, as the guided evaluation stacks it) -> the canvas eps
    ``[S, C, canvas_h, W]``, the guidance combine of ``groups`` evaluations folded in (``pf_window_merge``).  ``row_weight``: ``[win_h]``
    float32 on the device; ``scales``: ``()``, ``(s,)`` or ``(s1, s2)`` as ``guidance_plan`` returns them."""
    rows, ch, win_h, W = eps.shape
    if rows != groups * songs * n_windows:
        raise RuntimeError(f"window_merge: eps has {rows} rows, expected {groups} groups x {songs} songs x {n_windows} windows")
    if out is None:
        out = torch.empty(songs, ch, stride * (n_windows - 1) + win_h, W, dtype=torch.float32, device=eps.device)
    a = _lib.WindowMergeArgs()
    a.eps, a.row_weight, a.out, a.groups = eps.data_ptr(), row_weight.data_ptr(), out.data_ptr(), int(groups)
    a.s1, a.s2 = (float(v) for v in (tuple(scales) + (0.0, 0.0))[:2])
    a.songs, a.channels, a.win_h, a.width, a.n_windows, a.stride = songs, ch, win_h, W, int(n_windows), int(stride)
    _lib.check(lib.pf_window_merge(C.byref(a), _lib.current_stream()), "pf_window_merge", lib)
    return out


# ---- the training objective, forward only (LatentDiffusion.loss / DenoiseDiffusion.loss of the reference) -------------------------------
def sqrt_tables(alpha_bar: torch.Tensor, device):
    """``alpha_bar ** 0.5`` and ``(1 - alpha_bar) ** 0.5`` on the float32 ``alpha_bar``, as ``q_xt_x0`` / ``q_sample`` compute them
    (latent_diffusion.py:157-159, 177; ddpm/__init__.py:44-46, 64), as device tables for ``pf_qsample_rows``."""
    ab = alpha_bar.detach().to(device="cpu", dtype=torch.float32)
    # x ** 0.5 is the correctly rounded float32 square root where the host's float32 pow is IEEE-exact - and on some CPUs torch's
    # vectorised float32 pow is not (seen: one ulp at (1 - alpha_bar[999]) ** 0.5 of the ddpm schedule).  The float64 square root rounded
    # to float32 IS that value on every host (53 >= 2 * 24 + 2 bits: the double rounding is innocuous); 1 - alpha_bar stays a float32 operation.
    root = lambda v: torch.sqrt(v.double()).float()
    return root(ab).to(device).contiguous(), root(1 - ab).to(device).contiguous()


def time_steps(t, batch: int, n_steps: int, seed: int, device) -> torch.Tensor:
    """The ``t`` of a loss evaluation as a device int64 ``[batch]``.  ``None``: ``randint(0, n_steps)`` from a CPU generator seeded with
    ``seed`` (the reference draws on the device from the global generator, which nothing can pin).  A ``t`` held on the host - a
    sequence, a CPU tensor, or the one drawn here - is range-checked; a device tensor is taken as it is (the kernel clamps)."""
    if t is None:
        t = torch.randint(0, n_steps, (batch,), generator=torch.Generator().manual_seed(int(seed)), dtype=torch.int64)
    elif not isinstance(t, torch.Tensor):
        t = torch.as_tensor(t, dtype=torch.int64)
    if t.dim() != 1 or t.shape[0] != batch:
        raise RuntimeError(f"time steps of shape {tuple(t.shape)} for a batch of {batch}")
    if t.device.type == "cpu" and batch and (int(t.min()) < 0 or int(t.max()) >= n_steps):
        raise RuntimeError(f"time step outside [0, {n_steps}): {t.tolist()}")
    return t.to(device=device, dtype=torch.int64).contiguous()


def _rng_fields(args, rng):
    if rng is not None:
        args.rng = 1
        args.seed, args.draw, args.elem_offset = (int(v) for v in rng)


def qsample_rows(lib, x0, t, sqrt_ab, sqrt_1mab, *, noise=None, rng=None, noise_out=None, out=None) -> torch.Tensor:
    """``x_t[b] = sqrt_ab[t[b]] * x0[b] + sqrt_1mab[t[b]] * noise[b]`` (``pf_qsample_rows``).  ``noise``: a tensor like ``x0``, or
    ``rng = (seed, draw, elem_offset)``: drawn in the kernel (``noise_out``, optional, receives it).  ``t``: device int64 ``[B]``."""
    a = _lib.QsampleRowsArgs()
    if out is None:
        out = torch.empty_like(x0)
    a.x0, a.noise, a.t, a.x_t, a.noise_out = x0.data_ptr(), _lib.ptr(noise), t.data_ptr(), out.data_ptr(), _lib.ptr(noise_out)
    a.sqrt_ab, a.sqrt_1mab, a.n_steps = sqrt_ab.data_ptr(), sqrt_1mab.data_ptr(), sqrt_ab.numel()
    a.rows, a.row_elems = x0.shape[0], x0.numel() // max(1, x0.shape[0])
    _rng_fields(a, rng)
    _lib.check(lib.pf_qsample_rows(C.byref(a), _lib.current_stream()), "pf_qsample_rows", lib)
    return out


def mse_rows(lib, eps_theta, *, noise=None, rng=None) -> torch.Tensor:
    """``sum_i (noise[b, i] - eps_theta[b, i]) ** 2`` per sample as float64 ``[B]`` (``pf_mse_rows``); ``noise``: a tensor, or
    ``rng = (seed, draw, elem_offset)``: re-drawn in the kernel."""
    a = _lib.MseRowsArgs()
    rows, row_elems = eps_theta.shape[0], eps_theta.numel() // max(1, eps_theta.shape[0])
    out = torch.empty(rows, dtype=torch.float64, device=eps_theta.device)
    nb = int(lib.pf_mse_rows_workspace_bytes(rows, row_elems))
    ws = torch.empty(max(nb, 8) // 8, dtype=torch.float64, device=eps_theta.device)
    a.eps_theta, a.noise, a.row_sum, a.workspace, a.workspace_bytes = eps_theta.data_ptr(), _lib.ptr(noise), out.data_ptr(), ws.data_ptr(), nb
    a.rows, a.row_elems = rows, row_elems
    _rng_fields(a, rng)
    _lib.check(lib.pf_mse_rows(C.byref(a), _lib.current_stream()), "pf_mse_rows", lib)
    return out


def diffusion_loss_rows(lib, x0, t, tables, predict, *, noise=None, rng=None):
    """The body both ``loss`` methods share (latent_diffusion.py:226-240, ddpm/__init__.py:105-111): ``x_t = q_sample(x0, t, noise)``,
    ``eps_theta = predict(x_t)``, then the per-sample mean of ``(noise - eps_theta) ** 2`` as float64 ``[B]``.  Returns
    ``(loss_rows, x_t, eps_theta)``.  With ``rng`` the noise exists only inside the two kernels."""
    x0 = x0.contiguous().float()
    if noise is not None:
        noise = noise.to(device=x0.device, dtype=torch.float32).contiguous()
        if noise.shape != x0.shape:
            raise RuntimeError(f"noise of shape {tuple(noise.shape)} for x0 of shape {tuple(x0.shape)}")
        rng = None
    xt = qsample_rows(lib, x0, t, tables[0], tables[1], noise=noise, rng=rng)
    eps_theta = predict(xt).contiguous()
    if eps_theta.shape != x0.shape:
        raise RuntimeError(f"the model predicts {tuple(eps_theta.shape)} for noise of shape {tuple(x0.shape)}")
    rows = mse_rows(lib, eps_theta, noise=noise, rng=rng)
    return rows / float(x0.numel() // x0.shape[0]), xt, eps_theta
