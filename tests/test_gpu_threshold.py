"""Clipping and dynamic thresholding of the predicted x0 on the GPU (-m gpu).

ABI level - ``pf_x0_threshold`` against the numpy restatement in ``tests/threshold_ref.py``, everything bit for bit: ``eps_out`` as
``uint32``, ``q``, ``s``, ``w`` and the count as float64 bits, in both forms (resident and streamed) wherever the resident one is allowed,
on both access paths (16-byte vectors; single elements when a pointer is one float off, ``row_elems % 4 != 0`` or the stride of ``x`` is
odd), in place and out of place, with ``t`` differing per row at strides 1 and 3.  One stated exception to "bits": where a value is NaN,
both sides must hold a NaN at that place and its sign and payload are not compared - IEEE 754 leaves both to the implementation (the host
makes ``inf - inf`` a negative quiet NaN, the GPU a positive one).  Sentinels guard every buffer, the workspace included; inputs are read
only when out of place; a row alone is the row in its batch; two runs are identical.

Sampler level, on the small synthetic UNet of ``tests/test_gpu_guidance.py`` (32 x 32, so ``row_elems = 2048``): ``None`` is today's bits in
all three families, ``get_eps`` with the setting is ``_steps.x0_threshold`` of the plain ``get_eps``, two steps of each family are the loop
written by hand, a captured step is the eager loop and is keyed by the setting, ``cond_concat``, a window plan, ``DualScale`` with
``guidance_rescale``, and one CLI run."""
import ctypes as C
import functools
import math
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import dpm_ref  # noqa: E402
import threshold_ref as ref  # noqa: E402
from polyffusion_amd import _lib, _steps  # noqa: E402
from polyffusion_amd.arch import UNetConfig  # noqa: E402
from polyffusion_amd.sampler import DDIMSampler, DPMSolverSampler, DualScale, SDFSampler, WindowPlan, X0Threshold  # noqa: E402
from polyffusion_amd.unet import LatentDiffusion, UNetModel  # noqa: E402
from polyffusion_amd.weights import synth_unet_state  # noqa: E402

PAD = 8                 # elements of sentinel on either side of a buffer (the payload keeps its alignment)
SENTINEL = -777.25
F = np.float32
KINDS = ("noisy", "inside", "constant", "ties_inside", "ties_last", "nan", "inf")
T_VALUES = (0, 500, 999)
TABLE = ref.table_of(dpm_ref.alpha_bar().astype(F))
TABLE.setflags(write=False)


@pytest.fixture(scope="module")
def lib():
    _lib.require_gpu()
    return _lib.load()


def bits(t):
    a = t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def same(a, b):
    """Equality of bits, NaNs matching NaNs (module docstring)."""
    a, b = np.asarray(a), np.asarray(b)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(bits(a)[~na], bits(b)[~nb])


def padded(values, off=0, dtype=torch.float32):
    """(whole buffer, payload view) on the device: the payload starts `off` elements past a 16-byte boundary, sentinels around it."""
    values = np.asarray(values).reshape(-1)
    n = len(values)
    whole = torch.full((n + 2 * PAD + 4,), SENTINEL if dtype.is_floating_point else int(SENTINEL), device="cuda", dtype=dtype)
    assert whole.data_ptr() % 16 == 0
    view = whole[PAD + off: PAD + off + n]
    view.copy_(torch.from_numpy(values.copy()).to(dtype))
    return whole, view


def untouched(whole, n, off=0):
    w = whole.cpu().numpy()
    guard = SENTINEL if w.dtype.kind == "f" else int(SENTINEL)
    return bool((w[: PAD + off] == guard).all() and (w[PAD + off + n:] == guard).all())


def integral_p(n):
    """A p in (0, 1) whose product with n - 1 is a whole number in float64 (1.0 when the row is too short to have one)."""
    for j in range(max(1, (n - 1) // 2), n - 1):
        p = j / (n - 1)
        if p * (n - 1) == j:
            return p
    return 1.0


def p_values(n):
    return (0.5, 0.995, 1.0, 1e-9, integral_p(n))


@functools.lru_cache(maxsize=None)
def case(kind, rows, n, p, stride_extra=0):
    """(x [rows, n + stride_extra], eps [rows, n], t [rows]) float32 / int64 - computed once, shared, never written."""
    seed = 1000 * KINDS.index(kind) + 10 * rows + n % 97
    g = np.random.default_rng(seed)
    t = np.array([T_VALUES[(r + n) % 3] for r in range(rows)], np.int64)
    x, eps = np.empty((rows, n), F), np.empty((rows, n), F)
    k = int(math.floor(p * (n - 1)))
    for r in range(rows):
        cx, ce = TABLE[t[r], 0], TABLE[t[r], 1]
        ra, rb = F(1.0) / cx, ce / cx                                                # sqrt(ab), sqrt(1 - ab)
        noise = g.standard_normal(n).astype(F)
        if kind in ("noisy", "nan", "inf"):
            # a roll of 0 / 1 cells noised to time step t, and a prediction that is off: some cells of x0 leave [0, 1]
            x[r] = ra * (g.random(n) < 0.1).astype(F) + rb * noise
            eps[r] = noise + F(0.3) * g.standard_normal(n).astype(F)
        elif kind == "inside":
            x0 = g.uniform(0.05, 0.95, n).astype(F)
            eps[r] = noise
            x[r] = ((x0 + ce * noise) / cx).astype(F)
        elif kind == "constant":
            x[r], eps[r] = F(1.75 + r), F(-0.5)
        else:
            # four (x, eps) pairs, so four values of x0, in runs: the first run ends exactly at rank k (ties_last) or one past it (ties_inside)
            first = min(n, k + (1 if kind == "ties_last" else 2))
            ids = np.concatenate([np.zeros(first, np.int64), 1 + (np.arange(n - first) % 3)])
            g.shuffle(ids)
            x[r] = (np.array([2.0, 3.0, 5.0, 7.0], F) * ra)[ids]
            eps[r] = np.array([0.25, -0.5, 0.125, -1.0], F)[ids]
    if kind == "nan":
        eps[rows - 1, n // 2] = np.nan
    if kind == "inf":
        x[0, n // 3] = np.inf
    xs = np.full((rows, n + stride_extra), F(123.5))                                 # what lies behind a row's state is never read
    xs[:, :n] = x
    for a in (xs, eps, t):
        a.setflags(write=False)
    return xs, eps, t


def launch(lib, x, eps, out, t, table, rows, n, *, x_stride, t_stride=1, mode=1, form=0, p=0.995, s_max=math.inf, lo=0.0, hi=1.0, stats=None, ws=None,
           ws_bytes=None):
    a = _lib.X0ThresholdArgs()
    a.x, a.x_row_stride, a.eps, a.eps_out = x.data_ptr(), x_stride, eps.data_ptr(), out.data_ptr()
    a.t, a.t_stride, a.table, a.n_table = t.data_ptr(), t_stride, table.data_ptr(), table.numel() // 4
    a.stats, a.workspace = _lib.ptr(stats), _lib.ptr(ws)
    a.workspace_bytes = (0 if ws is None else ws.numel() * ws.element_size()) if ws_bytes is None else ws_bytes
    a.p, a.s_max, a.lo, a.hi, a.mode, a.form, a.rows, a.row_elems = p, s_max, lo, hi, mode, form, rows, n
    return lib.pf_x0_threshold(C.byref(a), _lib.current_stream())


def run_padded(lib, xs, eps, t, *, off=0, inplace=False, t_stride=1, want_stats=True, **kw):
    """One call on sentinel-guarded buffers; returns (eps_out [rows, n], stats [rows, 4] or None) as numpy, after checking every guard."""
    rows, n = eps.shape
    tt = np.full((rows - 1) * t_stride + 1, 7, np.int64)
    tt[::t_stride] = t
    x_w, x = padded(xs, off)
    e_w, e = padded(eps, off)
    o_w, o = (e_w, e) if inplace else padded(np.zeros(rows * n, F), off)
    t_w, td = padded(tt, 0, torch.int64)
    tb_w, tb = padded(TABLE, 0)
    st_w, st = padded(np.zeros(rows * 4), 0, torch.float64) if want_stats else (None, None)
    nws = int(lib.pf_x0_threshold_workspace_bytes(rows, n, kw.get("form", 0))) // 8
    ws_w, ws = padded(np.zeros(nws), 0, torch.int64) if nws else (None, None)
    _lib.check(launch(lib, x, e, o, td, tb, rows, n, x_stride=xs.shape[1], t_stride=t_stride, stats=st, ws=ws, **kw), "pf_x0_threshold", lib)
    torch.cuda.synchronize()
    assert untouched(x_w, xs.size, off) and untouched(o_w, rows * n, off) and untouched(e_w, rows * n, off) and untouched(t_w, tt.size)
    assert untouched(tb_w, TABLE.size) and (st_w is None or untouched(st_w, rows * 4)) and (ws_w is None or untouched(ws_w, nws))
    assert same(x.cpu().numpy(), xs.reshape(-1)) and np.array_equal(td.cpu().numpy(), tt) and np.array_equal(bits(tb), bits(TABLE.reshape(-1)))
    assert inplace or same(e.cpu().numpy(), eps.reshape(-1))                         # the inputs are read only
    return o.cpu().numpy().reshape(rows, n), None if st is None else st.cpu().numpy().reshape(rows, 4)


VARIANTS = [(off, extra, inplace, ts) for off in (0, 1) for extra in (0, 4, 3) for inplace in (False, True) for ts in (1, 3)]
SHAPES = [(rows, n) for rows in (1, 3) for n in (1, 2, 5, 2047, 2048, 2049, 4100)]


@pytest.mark.parametrize("rows,n", SHAPES)
def test_both_forms_are_the_restatement_bit_for_bit(lib, rows, n):
    """Every kind of row at every p, each with another variant of (alignment, stride of x, in place, stride of t): 35 cases walk the 24
    variants, so every shape meets every variant.  The first case of a shape runs twice; with three rows every row also runs alone."""
    i = rows + n
    for kind in KINDS:
        for p in p_values(n):
            off, extra, inplace, ts = VARIANTS[i % len(VARIANTS)]
            i += 1
            xs, eps, t = case(kind, rows, n, p, extra)
            want, wst = ref.threshold(xs, eps, t, TABLE, "dynamic", p=p)
            tag = (kind, rows, n, p, off, extra, inplace, ts)
            got = {form: run_padded(lib, xs, eps, t, off=off, inplace=inplace, t_stride=ts, form=form, p=p) for form in (1, 2)}
            for form, (out, st) in got.items():
                assert same(out, want), (tag, form, int((bits(out) != bits(want)).sum()))
                assert same(st, wst), (tag, form, st, wst)
            assert same(got[1][0], got[2][0]) and np.array_equal(bits(got[1][1]), bits(got[2][1])), tag      # the two forms: NaNs included
            auto = run_padded(lib, xs, eps, t, off=off, inplace=inplace, t_stride=ts, form=0, p=p)
            assert np.array_equal(bits(auto[0]), bits(got[1][0])) and np.array_equal(bits(auto[1]), bits(got[1][1])), tag   # and a second run
            # what the kinds are for
            if kind == "inside":
                assert (wst[:, 3] == 0).all() and same(want, eps), tag
            if kind in ("ties_inside", "constant") and n > 1:
                assert all(ref.order_stats(row, p)[2] == ref.order_stats(row, p)[3] for row in keys_of(xs, eps, t, n)), tag
            if kind == "ties_last" and math.floor(p * (n - 1)) + 1 < n:
                assert all(ref.order_stats(row, p)[2] < ref.order_stats(row, p)[3] for row in keys_of(xs, eps, t, n)), tag
            if kind == "noisy" and n >= 2047 and p >= 0.995:
                assert (wst[:, 0] > 0.5).all() and (wst[:, 2] < 1.0).all() and (wst[:, 3] > n // 2).all(), (tag, wst)
            if kind == "inf" and p == 1.0:
                assert not np.isfinite(wst[0, 0]) and np.isnan(wst[0, 1]) and wst[0, 3] == 0 and same(want[0], eps[0]), (tag, wst)
            print(f"{tag}: q {wst[:, 0]}, s {wst[:, 1]}, w {wst[:, 2]}, changed {wst[:, 3]}")
            if rows > 1 and kind in ("noisy", "ties_last") and p in (0.995, 1e-9):
                for r in range(rows):
                    for form in (1, 2):
                        o1, s1 = run_padded(lib, xs[r: r + 1], eps[r: r + 1], t[r: r + 1], off=off, form=form, p=p)
                        assert np.array_equal(bits(o1[0]), bits(got[form][0][r])) and np.array_equal(bits(s1[0]), bits(got[form][1][r])), (tag, r, form)


def keys_of(xs, eps, t, n):
    for r in range(eps.shape[0]):
        cx, ce = TABLE[t[r], 0], TABLE[t[r], 1]
        with np.errstate(all="ignore"):
            u = (((cx * xs[r, :n]).astype(F) - (ce * eps[r]).astype(F)) - F(0.5)).astype(F)
        yield u.view(np.uint32) & np.uint32(0x7FFFFFFF)


@pytest.mark.parametrize("n", [5, 2049, 4100])
def test_s_max_binds_another_range_and_time_steps_outside_the_table_are_clamped(lib, n):
    xs, eps, t = case("noisy", 3, n, 0.995)
    for form in (1, 2):
        want, wst = ref.threshold(xs, eps, t, TABLE, "dynamic", p=0.995, s_max=1.25)
        out, st = run_padded(lib, xs, eps, t, form=form, p=0.995, s_max=1.25)
        assert same(out, want) and same(st, wst)
        bound = wst[:, 0] > 0.625                                                    # (the row at t = 0 predicts x0 too well to reach the cap)
        assert n == 5 or (bound.sum() >= 2 and (wst[bound, 1] == 0.625).all() and (wst[bound, 2] == float(F(0.5 / 0.625))).all())
        want, wst = ref.threshold(xs, eps, t, TABLE, "dynamic", p=0.9, lo=-1.0, hi=1.0)
        out, st = run_padded(lib, xs, eps, t, form=form, p=0.9, lo=-1.0, hi=1.0)
        assert same(out, want) and same(st, wst)
        far = np.array([-3, 1000, 2 ** 40], np.int64)
        want, wst = ref.threshold(xs, eps, far, TABLE, "dynamic", p=0.995)
        out, st = run_padded(lib, xs, eps, far, form=form, p=0.995)
        assert same(out, want) and same(st, wst)


@pytest.mark.parametrize("rows,n", [(1, 1), (3, 5), (3, 2048), (1, 2049), (3, 4100)])
def test_clip_mode_with_and_without_stats(lib, rows, n):
    for kind in ("noisy", "inside", "nan", "inf"):
        for i, (off, extra, inplace, ts) in enumerate(VARIANTS[(rows + n) % 5::5]):
            xs, eps, t = case(kind, rows, n, 0.995, extra)
            want, wst = ref.threshold(xs, eps, t, TABLE, "clip")
            assert np.isnan(wst[:, :2]).all() and (wst[:, 2] == 1.0).all()
            for form in (1, 2):
                out, st = run_padded(lib, xs, eps, t, off=off, inplace=inplace, t_stride=ts, form=form, mode=0)
                assert same(out, want) and same(st, wst), (kind, rows, n, off, extra, inplace, ts, form)
                bare, none = run_padded(lib, xs, eps, t, off=off, inplace=inplace, t_stride=ts, form=form, mode=0, want_stats=False)
                assert none is None and np.array_equal(bits(bare), bits(out))
            if kind == "noisy" and n >= 2048:
                assert (wst[:, 3] > 0).all() and (wst[:, 3] < n).all()
    xs, eps, t = case("noisy", rows, n, 0.995)
    out, _ = run_padded(lib, xs, eps, t, form=2, p=0.995, want_stats=False)         # dynamic without stats
    assert same(out, ref.threshold(xs, eps, t, TABLE, "dynamic", p=0.995)[0])


def test_the_products_row_runs_the_resident_form_at_its_lds_limit(lib):
    n = _lib.X0T_RESIDENT_MAX
    xs, eps, t = case("noisy", 2, n, 0.995)
    want, wst = ref.threshold(xs, eps, t, TABLE, "dynamic", p=0.995)
    assert (wst[:, 0] > 0.5).all()
    for form in (0, 1, 2):
        out, st = run_padded(lib, xs, eps, t, form=form, p=0.995)
        assert same(out, want) and same(st, wst), form
    assert lib.pf_x0_threshold_workspace_bytes(2, n, 0) == 0 and lib.pf_x0_threshold_workspace_bytes(2, n + 1, 0) > 0
    xs, eps, t = case("noisy", 1, n + 4, 0.995)                                      # one group more: auto streams
    out, st = run_padded(lib, xs, eps, t, form=0, p=0.995)
    want, wst = ref.threshold(xs, eps, t, TABLE, "dynamic", p=0.995)
    assert same(out, want) and same(st, wst)


def test_refusals_launch_nothing(lib):
    rows, n = 2, 2049
    x, eps = torch.zeros(rows * n + 8, device="cuda"), torch.zeros(rows * n + 8, device="cuda")
    out = torch.full((rows * n + 8,), SENTINEL, device="cuda")
    t, table = torch.zeros(rows, dtype=torch.int64, device="cuda"), torch.from_numpy(TABLE.copy()).cuda()
    stats = torch.full((rows * 4 + 1,), SENTINEL, device="cuda", dtype=torch.float64)
    need = int(lib.pf_x0_threshold_workspace_bytes(rows, n, 2))
    ws = torch.full((need // 8 + 1,), -7, device="cuda", dtype=torch.int64)

    def refused(pattern, **kw):
        a = dict(x=x, eps=eps, out=out, t=t, table=table, rows=rows, n=n, x_stride=n, form=2, stats=stats, ws=ws, ws_bytes=need)
        a.update(kw)
        rc = launch(lib, **a)
        msg = lib.pf_last_error().decode()
        assert rc == -1 and msg.startswith("x0_threshold: ") and pattern in msg, (kw, rc, msg)

    refused("0 rows", rows=0)
    refused("x_row_stride 2048 below row_elems 2049", x_stride=n - 1)
    refused("outside (0, 1]", p=0.0)
    refused("below 1", s_max=0.5)
    refused("is not lo < hi", lo=1.0, hi=0.0)
    refused("unknown mode 2", mode=2)
    refused("unknown form 3", form=3)
    refused("the resident form holds rows of at most 32768", form=1, n=40000, x_stride=40000)
    refused("eps_out overlaps eps partially", out=eps[1:])
    refused("eps_out overlaps x", out=x)
    refused("no workspace", ws=None)
    refused(f"workspace of {need} bytes required, got {need - 8}", ws_bytes=need - 8)
    refused("workspace must be 8-byte aligned", ws=ws.view(torch.int32)[1:])
    refused("stats must be 8-byte aligned", stats=stats.view(torch.float32)[1:])
    torch.cuda.synchronize()
    assert (out == SENTINEL).all() and (stats == SENTINEL).all() and (ws == -7).all()


# ---------------------------------------------------------------------------------------------- the samplers
def small(in_channels=2):
    kw = dict(in_channels=in_channels, out_channels=2, channels=32, n_res_blocks=1, attention_levels=(1,), channel_multipliers=(1, 2), n_heads=2,
              tf_layers=1, d_cond=32)
    m = UNetModel(img_h=32, img_w=32, **kw)
    m.load_state_dict(synth_unet_state(UNetConfig(**kw), 0))
    return m


@pytest.fixture(scope="module")
def net():
    _lib.require_gpu()
    return small()


def inputs(rows=2, h=32):
    g = torch.Generator().manual_seed(9)
    x, c = torch.randn(rows, 2, h, 32, generator=g).cuda(), torch.randn(2 * rows, 1, 32, generator=g)[:rows].cuda()
    return x, c, -torch.ones_like(c)


FAMILIES = {
    "ddpm": lambda ldm, **kw: SDFSampler(ldm, seed=3, **kw),
    "ddim": lambda ldm, **kw: DDIMSampler(ldm, 20, "uniform", 0.0, seed=3, **kw),
    "dpm": lambda ldm, **kw: DPMSolverSampler(ldm, 6, seed=3, **kw),
}
SCALE = 5.0
SPLIT = 12
TH = X0Threshold("dynamic", 0.995)


def by_hand(lib, s, th):
    """``s`` (built without the setting) with its ``get_eps`` followed by ``_steps.x0_threshold``: the loop written by hand."""
    plain = s.get_eps

    def get_eps(x, t, c, **kw):
        e = plain(x, t, c, **kw)
        wp = s.windows
        return _steps.x0_threshold(lib, x.contiguous(), e.contiguous(), t, s.model.x0_threshold_table(x.device), mode=th.mode, p=th.p, range=th.range,
                                   s_max=th.s_max, t_stride=1 if wp is None else wp.n_windows)[0]
    s.get_eps = get_eps
    return s


@pytest.mark.parametrize("family", list(FAMILIES))
def test_none_is_todays_bits_and_two_steps_are_the_loop_written_by_hand(lib, net, family):
    x, c, uc = inputs()
    kw = dict(uncond_scale=SCALE, uncond_cond=uc)
    plain = FAMILIES[family](LatentDiffusion(net)).paint(x, c, 1, **kw)
    s = FAMILIES[family](LatentDiffusion(net), x0_threshold=None)
    assert torch.equal(s.paint(x, c, 1, **kw), plain) and s.last_threshold is None
    for th in (TH, X0Threshold("clip"), X0Threshold("dynamic", 0.9, (-1.0, 1.0), 2.0)):
        s = FAMILIES[family](LatentDiffusion(net), x0_threshold=th)
        got = s.paint(x, c, 1, **kw)
        assert torch.isfinite(got).all() and not torch.equal(got, plain)
        assert s.last_threshold.shape == (2, 4) and s.last_threshold.dtype == torch.float64 and (s.last_threshold[:, 3] > 0).all()
        assert torch.equal(got, by_hand(lib, FAMILIES[family](LatentDiffusion(net)), th).paint(x, c, 1, **kw))
    # independent of the interval: a step outside it is thresholded too
    taus = FAMILIES[family](LatentDiffusion(net)).time_steps[:2]
    s = FAMILIES[family](LatentDiffusion(net), x0_threshold=TH, guidance_interval=(int(taus[1]), int(taus[1])))
    want = by_hand(lib, FAMILIES[family](LatentDiffusion(net), guidance_interval=(int(taus[1]), int(taus[1]))), TH).paint(x, c, 1, **kw)
    assert torch.equal(s.paint(x, c, 1, **kw), want)


def test_get_eps_with_the_setting_is_x0_threshold_of_the_plain_get_eps(lib, net):
    x, c, uc = inputs()
    ldm = LatentDiffusion(net)
    t = torch.tensor([500, 200]).cuda()
    table = ldm.x0_threshold_table(x.device)
    assert np.array_equal(bits(table), bits(ref.table_of(ldm.alpha_bar.numpy())))
    for th in (TH, X0Threshold("clip")):
        for scale, phi in ((SCALE, 0.0), (1.0, 0.0), (DualScale(3.0, 5.0, SPLIT), 0.7), (SCALE, 0.7)):      # DualScale together with guidance_rescale
            plain = SDFSampler(ldm, seed=3, guidance_rescale=phi).get_eps(x, t, c, uncond_scale=scale, uncond_cond=uc).clone()
            want, st = _steps.x0_threshold(lib, x, plain, t, table, mode=th.mode, p=th.p, want_stats=True)
            s = SDFSampler(ldm, seed=3, guidance_rescale=phi, x0_threshold=th)
            got = s.get_eps(x, t, c, uncond_scale=scale, uncond_cond=uc)
            assert torch.equal(got, want) and np.array_equal(bits(s.last_threshold), bits(st)) and not torch.equal(got, plain)
            rwant, rst = ref.threshold(x.cpu().numpy().reshape(2, -1), plain.cpu().numpy().reshape(2, -1), t.cpu().numpy(), ref.table_of(ldm.alpha_bar.numpy()),
                                       th.mode, p=th.p)
            assert same(got.cpu().numpy().reshape(2, -1), rwant) and same(st.cpu().numpy(), rst)
            assert st[0, 0] != st[1, 0] or th.mode == "clip"                      # each row its own time step and its own quantile


@pytest.mark.parametrize("family", list(FAMILIES))
def test_a_captured_step_is_the_eager_loop_and_is_keyed_by_the_setting(net, family):
    x, c, uc = inputs()

    def paint(s):
        s._draws = 0                                                                # every run from the sampler's first draw (DDPM draws per step)
        return s.paint(x, c, 2, uncond_scale=SCALE, uncond_cond=uc)

    eager = FAMILIES[family](LatentDiffusion(net), x0_threshold=TH).paint(x, c, 2, uncond_scale=SCALE, uncond_cond=uc)
    s = FAMILIES[family](LatentDiffusion(net), graph=True, x0_threshold=TH)
    assert torch.equal(paint(s), eager) and s.graph_captures == 1
    s.x0_threshold = X0Threshold("dynamic", 0.995)                                  # an equal setting: the same capture
    assert torch.equal(paint(s), eager) and s.graph_captures == 1
    s.x0_threshold = X0Threshold("clip")
    other = paint(s)
    assert s.graph_captures == 2 and not torch.equal(other, eager)
    assert torch.equal(other, FAMILIES[family](LatentDiffusion(net), x0_threshold=X0Threshold("clip")).paint(x, c, 2, uncond_scale=SCALE, uncond_cond=uc))
    s.x0_threshold = None
    assert torch.equal(paint(s), FAMILIES[family](LatentDiffusion(net)).paint(x, c, 2, uncond_scale=SCALE, uncond_cond=uc)) and s.graph_captures == 3


def test_cond_concat_channels_lie_behind_the_state_and_are_not_read(lib):
    ldm = LatentDiffusion(small(in_channels=4))
    x, c, uc = inputs()
    cc = torch.randn(2, 2, 32, 32, generator=torch.Generator().manual_seed(5)).cuda() * 50.0
    xin = torch.cat([x, cc], dim=1)
    t = torch.tensor([700, 300]).cuda()
    plain = DDIMSampler(ldm, 20, "uniform", 0.0, seed=3).get_eps(xin, t, c, uncond_scale=SCALE, uncond_cond=uc).clone()
    assert plain.shape == (2, 2, 32, 32)
    s = DDIMSampler(ldm, 20, "uniform", 0.0, seed=3, x0_threshold=TH)
    got = s.get_eps(xin, t, c, uncond_scale=SCALE, uncond_cond=uc)
    rwant, rst = ref.threshold(x.cpu().numpy().reshape(2, -1), plain.cpu().numpy().reshape(2, -1), t.cpu().numpy(), ref.table_of(ldm.alpha_bar.numpy()), "dynamic")
    assert same(got.cpu().numpy().reshape(2, -1), rwant) and same(s.last_threshold.cpu().numpy(), rst)
    # and through a loop: paint concatenates the channels itself
    out = s.paint(x, c, 1, uncond_scale=SCALE, uncond_cond=uc, cond_concat=cc)
    assert torch.equal(out, by_hand(lib, DDIMSampler(ldm, 20, "uniform", 0.0, seed=3), TH).paint(x, c, 1, uncond_scale=SCALE, uncond_cond=uc, cond_concat=cc))


def test_a_window_plan_thresholds_the_canvas_with_the_first_windows_time_step(lib, net):
    wp = WindowPlan(2, 16, 32)
    x, c, uc = inputs(2, wp.canvas_h)[0], inputs(4)[1], inputs(4)[2]               # two songs of two windows each: canvases, one condition row per window
    ldm = LatentDiffusion(net)
    t = torch.tensor([500, 100, 300, 900]).cuda()                                  # (the loops feed every window the same value; the rule is the first one's)
    plain = DDIMSampler(ldm, 20, "uniform", 0.0, seed=3, windows=wp).get_eps(x, t, c, uncond_scale=SCALE, uncond_cond=uc).clone()
    assert plain.shape == (2, 2, wp.canvas_h, 32)
    s = DDIMSampler(ldm, 20, "uniform", 0.0, seed=3, windows=wp, x0_threshold=TH)
    got = s.get_eps(x, t, c, uncond_scale=SCALE, uncond_cond=uc)
    rwant, rst = ref.threshold(x.cpu().numpy().reshape(2, -1), plain.cpu().numpy().reshape(2, -1), np.array([500, 300]), ref.table_of(ldm.alpha_bar.numpy()), "dynamic")
    assert same(got.cpu().numpy().reshape(2, -1), rwant) and s.last_threshold.shape == (2, 4) and same(s.last_threshold.cpu().numpy(), rst)
    out = s.paint(x, c, 1, uncond_scale=SCALE, uncond_cond=uc)
    hand = by_hand(lib, DDIMSampler(ldm, 20, "uniform", 0.0, seed=3, windows=wp), TH)
    assert torch.equal(out, hand.paint(x, c, 1, uncond_scale=SCALE, uncond_cond=uc))


# ---------------------------------------------------------------------------------------------- the CLI
def test_cli_writes_a_stamp_that_names_the_setting(tmp_path):
    from polyffusion_amd import inference_sdf
    out = tmp_path / "a"
    argv = ["--params_preset", "sdf_chd8bar", "--synthetic_weights", "--synthetic", "--length", "1", "--ddim", "--ddim_steps", "4",
            "--uncond_scale", "5", "--x0_threshold", "0.995", "--seed", "7", "--output_dir", str(out)]
    assert inference_sdf.main(argv) == 0
    mids = [f for f in os.listdir(out) if f.endswith(".mid")]
    npys = [f for f in os.listdir(out) if f.endswith(".npy")]
    assert len(mids) == 1 and len(npys) == 1 and os.path.getsize(out / mids[0]) > 0
    assert "[scale=5.0,x0thr=0.995]" in mids[0] and "[scale=5.0,x0thr=0.995]" in npys[0] and mids[0].startswith("sdf_chd8bar")
    roll = np.load(out / npys[0])
    assert np.isfinite(roll).all() and roll.shape == (1, 2, 128, 128)
