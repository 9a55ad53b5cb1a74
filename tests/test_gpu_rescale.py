"""Guidance rescale and the guidance interval on the GPU (-m gpu).

ABI level - ``pf_cfg_rescale`` against the numpy restatement in ``tests/rescale_ref.py`` on both of its paths (16-byte vectors, and single
elements when a pointer is off by one float or ``row_elems % 4 != 0``): the four row sums the call leaves in its workspace (double-double partials, added as the kernel adds them) against
``math.fsum``, ``w`` against the restatement's, ``out`` bit for bit ``float32(e_cfg * w)`` with the ``w`` the kernel reports, sentinels around
every buffer, a row alone against the row in its batch, two runs, the refusals.

Bounds.  A sum: ``2^-52 * sum |term|``.  ``w``: one float32 ulp (both sides round a float64 that agrees to about 2^-45 even on the rows with
mean 10, where the variance loses seven bits to cancellation).  Everything else is equality of bits.

Sampler level, on the small synthetic UNet of ``tests/test_gpu_guidance.py`` (32 x 32, 32 channels): the two settings at their defaults are
today's bits in every family, ``get_eps`` with phi is ``_steps.cfg_rescale`` of the stacked forward, a captured step with phi is the eager
loop and is keyed by phi, a run with an interval is the hand-written loop that switches the scale (and the denoiser sees B rows outside
the interval, G * B inside), a window plan rescales per window and merges plainly, ``DualScale`` with phi, and one CLI run."""
import ctypes as C
import functools
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import rescale_ref  # noqa: E402
from polyffusion_amd import _lib, _steps  # noqa: E402
from polyffusion_amd.arch import UNetConfig  # noqa: E402
from polyffusion_amd.sampler import DDIMSampler, DPMSolverSampler, DualScale, SDFSampler, WindowPlan, guidance_plan  # noqa: E402
from polyffusion_amd.unet import LatentDiffusion, UNetModel  # noqa: E402
from polyffusion_amd.weights import synth_unet_state  # noqa: E402

PAD = 8                 # elements of sentinel on either side of a buffer (the payload keeps its alignment)
SENTINEL = -777.25
PHI = 0.7
SPLIT = 12              # chord part of the 32-wide condition of the small UNet
KINDS = ("normal", "mean10", "constant", "zero_scale")


@pytest.fixture(scope="module")
def lib():
    _lib.require_gpu()
    return _lib.load()


def bits(t):
    a = t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def padded(values, off=0, dtype=torch.float32):
    """(whole buffer, payload view) on the device: the payload starts `off` elements past a 16-byte boundary, sentinels around it."""
    values = np.asarray(values).reshape(-1)
    n = len(values)
    whole = torch.full((n + 2 * PAD + 4,), SENTINEL, device="cuda", dtype=dtype)
    assert whole.data_ptr() % 16 == 0
    view = whole[PAD + off: PAD + off + n]
    view.copy_(torch.from_numpy(values.copy()).to(dtype))
    return whole, view


def untouched(whole, n, off=0):
    w = whole.cpu().numpy()
    return bool((w[: PAD + off] == SENTINEL).all() and (w[PAD + off + n:] == SENTINEL).all())


@functools.lru_cache(maxsize=None)
def case(kind, groups, rows, n):
    """(epsg [G, rows, n] float32, s1, s2, the restatement's result) - computed once, shared by every test, never written."""
    seed = 1000 * KINDS.index(kind) + 100 * groups + 10 * rows + n % 7
    g = np.random.default_rng(seed).standard_normal((groups, rows, n)).astype(np.float32)
    s1, s2 = (5.0, 0.0) if groups == 2 else (3.0, 5.0)
    if kind == "mean10":
        g = (g + np.float32(10.0)).astype(np.float32)
    elif kind == "constant":                    # every group the same constant per row: var_pos == var_cfg == 0 exactly (sums of n * 2.25 are exact)
        g[:] = (np.float32(1.5) + np.arange(rows, dtype=np.float32)).reshape(1, rows, 1)
    elif kind == "zero_scale":                  # e_cfg = e_u + 0 * (...) = the constant e_u: var_cfg == 0 < var_pos
        s1, s2 = 0.0, 0.0
        g[0] = np.float32(0.5)
    g.setflags(write=False)
    ref = rescale_ref.rescale(g, s1, s2, PHI)
    return g, s1, s2, ref


def launch(lib, epsg_dev, out_dev, groups, rows, n, s1, s2, phi, ws, stats=None, weights=None, ws_bytes=None):
    a = _lib.CfgRescaleArgs()
    a.epsg, a.eps, a.stats, a.weights = epsg_dev.data_ptr(), out_dev.data_ptr(), _lib.ptr(stats), _lib.ptr(weights)
    a.workspace, a.workspace_bytes = _lib.ptr(ws), (0 if ws is None else ws.numel() * 8) if ws_bytes is None else ws_bytes
    a.phi, a.s1, a.s2, a.groups, a.rows, a.row_elems = phi, s1, s2, groups, rows, n
    return lib.pf_cfg_rescale(C.byref(a), _lib.current_stream())


def run_padded(lib, g, s1, s2, off, phi=PHI):
    """One call on sentinel-guarded buffers; returns out, stats, weights, workspace as numpy and whether every guard survived."""
    groups, rows, n = g.shape
    src_w, src = padded(g, off)
    out_w, out = padded(np.zeros(rows * n, np.float32), off)
    st_w, st = padded(np.zeros(rows * 3), 0, torch.float64)
    wt_w, wt = padded(np.zeros(rows, np.float32), 0)
    nws = int(lib.pf_cfg_rescale_workspace_bytes(rows, n)) // 8
    ws_w, ws = padded(np.zeros(nws), 0, torch.float64)
    _lib.check(launch(lib, src, out, groups, rows, n, s1, s2, phi, ws, st, wt), "pf_cfg_rescale", lib)
    torch.cuda.synchronize()
    guards = (untouched(out_w, rows * n, off) and untouched(src_w, g.size, off) and untouched(st_w, rows * 3) and untouched(wt_w, rows)
              and untouched(ws_w, nws))
    assert np.array_equal(src.cpu().numpy(), g.reshape(-1))                      # the input is read only
    return out.cpu().numpy().reshape(rows, n), st.cpu().numpy().reshape(rows, 3), wt.cpu().numpy(), ws.cpu().numpy().reshape(rows, -1, 4, 2), guards


def ulps_apart(a, b):
    return np.abs(np.asarray(a, np.float32).view(np.int32).astype(np.int64) - np.asarray(b, np.float32).view(np.int32).astype(np.int64))


_RUNS = {}


def run_case(lib, kind, groups, rows, n, off):
    """``run_padded`` of a case, once per module: the two tests below look at the same launches."""
    key = (kind, groups, rows, n, off)
    if key not in _RUNS:
        g, s1, s2, _ = case(kind, groups, rows, n)
        _RUNS[key] = run_padded(lib, g, s1, s2, off)
    return _RUNS[key]


chunk_order_sums = rescale_ref.chunk_order_sums


SHAPES = [(rows, groups, n) for rows in (1, 3) for groups in (2, 3) for n in (1, 3, 2048, 2049, 4100, 32768)]


@pytest.mark.parametrize("rows,groups,n", SHAPES)
def test_the_four_sums_against_fsum(lib, rows, groups, n):
    """Each sum within ``2^-52 * sum |term|`` of ``math.fsum`` of the same float64 terms - between one and two ulps of a sum of one sign.

    The kernel adds in the library's fixed order (8 terms per lane, a 6-level butterfly, 4 waves, then the chunks) with every addition in
    double-double, and rounds the total once: the correctly rounded sum but for near-ties, at most one ulp from ``fsum``.  Plain float64
    additions in the same order were measured on an MI355X at one to two ulps off on the sums of squares - one input of the 96 here
    (zero scale, rows 1, groups 3, n 2049: |err| 4.547e-13 = two ulps of 1995 against a bound of 4.429e-13) outside this bound - which
    is why the sums carry their rounding errors."""
    worst_of = {}
    for kind in KINDS:
        ref = case(kind, groups, rows, n)[3]
        for off in (0, 1):
            ws = run_case(lib, kind, groups, rows, n, off)[3]
            err, bound = np.abs(chunk_order_sums(ws) - ref["sums"]), 2.0 ** -52 * ref["mags"]
            with np.errstate(divide="ignore", invalid="ignore"):
                worst_of[kind, off] = float(np.nanmax(np.where(bound > 0, err / bound, np.where(err > 0, np.inf, 0.0))))
            print(f"{(kind, rows, groups, n, off)}: sums |err| / bound {worst_of[kind, off]:.3f}, |err| {err.max(axis=0)}, bound {bound.min(axis=0)}")
    assert all(v <= 1.0 for v in worst_of.values()), worst_of


@pytest.mark.parametrize("rows,groups,n", SHAPES)
def test_rescale_is_its_definition_on_both_paths(lib, rows, groups, n):
    chunks = -(-n // _lib.MSE_CHUNK)
    assert lib.pf_cfg_rescale_workspace_bytes(rows, n) == rows * chunks * 64
    for kind in KINDS:
        g, s1, s2, ref = case(kind, groups, rows, n)
        # the restatement's e_cfg is what the plain combine launches write for this input
        src = torch.from_numpy(g.reshape(-1).copy()).cuda()
        plain = torch.empty(rows * n, device="cuda")
        if groups == 2:
            _lib.check(lib.pf_cfg_combine(src.data_ptr(), s1, plain.data_ptr(), rows * n, _lib.current_stream()), "pf_cfg_combine")
        else:
            _lib.check(lib.pf_cfg_combine3(src.data_ptr(), s1, s2, plain.data_ptr(), rows * n, _lib.current_stream()), "pf_cfg_combine3")
        assert np.array_equal(bits(plain), bits(ref["e_cfg"].reshape(-1))), (kind, "e_cfg")
        first = None
        for off in (0, 1):
            out, stats, w, ws, guards = run_case(lib, kind, groups, rows, n, off)
            tag = (kind, rows, groups, n, off)
            assert guards, tag
            assert (ulps_apart(w, ref["w"]) <= 1).all(), (tag, w, ref["w"])
            assert np.array_equal(bits(out), bits(rescale_ref.scale_rows(ref["e_cfg"], w))), tag
            # the table is what the kernel's own sums give: var to a few roundings of its larger term, f the root of the table's quotient
            sums = chunk_order_sums(ws)
            vp, vc, f, _ = rescale_ref.factors(sums, n, PHI)
            assert (np.abs(stats[:, 0] - vp) <= 2.0 ** -50 * np.abs(sums[:, 1] / n)).all() and (np.abs(stats[:, 1] - vc) <= 2.0 ** -50 * np.abs(sums[:, 3] / n)).all()
            assert np.allclose(stats[:, 2], f, rtol=2.0 ** -40, atol=0.0), (tag, stats[:, 2], f)
            if kind in ("constant", "zero_scale"):
                assert (stats[:, 1] == 0.0).all() and (stats[:, 2] == 1.0).all() and (w == 1.0).all(), (tag, stats)
                assert np.array_equal(bits(out), bits(ref["e_cfg"])), tag                 # f = 1: e_cfg bit for bit
                assert kind == "constant" or n == 1 or (stats[:, 0] > 0).all()
            elif n >= 2048:
                assert (stats[:, 1] > stats[:, 0]).all() and (w < 1.0).all() and (w > 1.0 - PHI).all(), (tag, stats, w)
            # vectors or single elements: the same bits; and a second run too
            if first is None:
                first = (out, stats, w, ws)
                again = run_padded(lib, g, s1, s2, off)
                assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(first, again[:4])), tag
            else:
                assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(first, (out, stats, w, ws))), tag
        # every row computed alone is that row computed in the batch
        if rows > 1:
            for r in range(rows):
                o1, st1, w1, ws1, guards = run_padded(lib, np.ascontiguousarray(g[:, r: r + 1]), s1, s2, 0)
                assert guards and np.array_equal(bits(o1[0]), bits(first[0][r])) and np.array_equal(bits(st1[0]), bits(first[1][r]))
                assert np.array_equal(bits(w1), bits(first[2][r: r + 1])) and np.array_equal(bits(ws1[0]), bits(first[3][r]))


def test_phi_zero_is_the_plain_combine_and_the_tables_are_optional(lib):
    g, s1, s2, ref = case("normal", 3, 3, 2049)
    out, stats, w, _, guards = run_padded(lib, g, s1, s2, 0, phi=0.0)
    assert guards and (w == 1.0).all() and np.array_equal(bits(out), bits(ref["e_cfg"]))
    assert (stats[:, 2] != 1.0).all()                                               # f is reported all the same
    full, _, _, _, _ = run_padded(lib, g, s1, s2, 0)
    src = torch.from_numpy(g.reshape(-1).copy()).cuda()
    o = torch.full((3 * 2049,), SENTINEL, device="cuda")
    ws = _steps.cfg_rescale_workspace(lib, 3, 2049, "cuda")
    _lib.check(launch(lib, src, o, 3, 3, 2049, s1, s2, PHI, ws), "pf_cfg_rescale", lib)         # stats = weights = NULL
    assert np.array_equal(bits(o), bits(full.reshape(-1)))


def test_refusals_launch_nothing(lib):
    rows, n, groups = 2, 2049, 2
    src = torch.zeros(groups * rows * n + 8, device="cuda")
    out = torch.full((rows * n + 8,), SENTINEL, device="cuda")
    stats = torch.full((rows * 3 + 1,), SENTINEL, device="cuda", dtype=torch.float64)
    wts = torch.full((rows,), SENTINEL, device="cuda")
    ws = torch.full((rows * 2 * 8 + 1,), SENTINEL, device="cuda", dtype=torch.float64)
    need = int(lib.pf_cfg_rescale_workspace_bytes(rows, n))
    assert need == rows * 2 * 64

    def refused(pattern, **kw):
        a = dict(epsg_dev=src, out_dev=out, groups=groups, rows=rows, n=n, s1=5.0, s2=0.0, phi=PHI, ws=ws, stats=stats, weights=wts, ws_bytes=need)
        a.update(kw)
        rc = launch(lib, **a)
        msg = lib.pf_last_error().decode()
        assert rc == -1 and msg.startswith("cfg_rescale:") and pattern in msg, (kw, rc, msg)

    class Null:
        @staticmethod
        def data_ptr():
            return None

    refused("null epsg or eps", epsg_dev=Null)
    refused("null epsg or eps", out_dev=Null)
    for bad in (1, 4, 0, -2):
        refused(f"groups {bad}", groups=bad)
    refused("0 rows", rows=0)
    refused("of 0 elements", n=0)
    for bad in (-0.1, 1.5, float("nan"), float("inf")):
        refused("outside [0, 1]", phi=bad)
    refused("eps overlaps epsg", out_dev=src)
    refused("eps overlaps epsg", out_dev=src[groups * rows * n - 1:])               # the last element only
    refused("no workspace", ws=None)
    refused(f"workspace of {need} bytes required, got {need - 8}", ws_bytes=need - 8)
    refused("workspace must be 8-byte aligned", ws=ws.view(torch.float32)[1:])
    refused("stats must be 8-byte aligned", stats=stats.view(torch.float32)[1:])
    refused("more workgroups than one launch holds", rows=2 ** 30, ws_bytes=2 ** 62)
    torch.cuda.synchronize()
    for buf in (out, stats, wts, ws):
        assert (buf == SENTINEL).all()
    assert lib.pf_cfg_rescale(None, None) == -1 and lib.pf_last_error().decode().startswith("cfg_rescale:")


# ---------------------------------------------------------------------------------------------- the samplers
def small():
    kw = dict(in_channels=2, out_channels=2, channels=32, n_res_blocks=1, attention_levels=(1,), channel_multipliers=(1, 2), n_heads=2,
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


@pytest.mark.parametrize("family", list(FAMILIES))
def test_the_defaults_are_a_sampler_built_without_the_keywords(net, family):
    x, c, uc = inputs()
    plain = FAMILIES[family](LatentDiffusion(net)).paint(x, c, 3, uncond_scale=SCALE, uncond_cond=uc)
    for kw in (dict(guidance_rescale=0.0, guidance_interval=None), dict(guidance_rescale=0, guidance_interval=(0, 999))):
        s = FAMILIES[family](LatentDiffusion(net), **kw)
        assert torch.equal(s.paint(x, c, 3, uncond_scale=SCALE, uncond_cond=uc), plain) and s.last_rescale is None
    s = FAMILIES[family](LatentDiffusion(net), guidance_rescale=PHI)
    scaled = s.paint(x, c, 3, uncond_scale=SCALE, uncond_cond=uc)
    assert torch.isfinite(scaled).all() and not torch.equal(scaled, plain)
    stats, weights = s.last_rescale
    assert stats.shape == (2, 3) and stats.dtype == torch.float64 and weights.shape == (2,) and weights.dtype == torch.float32
    assert (weights > 1.0 - PHI).all() and (weights < 1.0).all()
    # one group has nothing to rescale: scale 1, scale 0 and no uncond_cond ignore phi
    for kw in (dict(uncond_scale=1.0, uncond_cond=uc), dict(uncond_scale=0.0, uncond_cond=uc), dict(uncond_scale=SCALE, uncond_cond=None)):
        a = FAMILIES[family](LatentDiffusion(net), guidance_rescale=PHI)
        assert torch.equal(a.paint(x, c, 3, **kw), FAMILIES[family](LatentDiffusion(net)).paint(x, c, 3, **kw)) and a.last_rescale is None


def test_get_eps_with_phi_is_cfg_rescale_of_the_stacked_forward(lib, net):
    x, c, uc = inputs()
    ldm = LatentDiffusion(net)
    s = SDFSampler(ldm, seed=3, guidance_rescale=PHI)
    t = torch.tensor([500, 500]).cuda()
    for scale in (SCALE, DualScale(3.0, 5.0, SPLIT), DualScale(3.0, 5.0, SPLIT, "txt,chd")):
        ctx, groups, scales = guidance_plan(c, scale, uc)
        assert groups == (2 if scale == SCALE else 3)
        eg = ldm(x, torch.cat([t] * groups), ctx, shared_x=True if groups == 2 else groups).clone()
        want, st, wt = _steps.cfg_rescale(lib, eg, groups, scales, PHI, want_stats=True)
        got = s.get_eps(x, t, c, uncond_scale=scale, uncond_cond=uc)
        assert torch.equal(got, want) and torch.equal(s.last_rescale[0], st) and torch.equal(s.last_rescale[1], wt)
        assert torch.equal(s.get_eps(x, t, c, uncond_scale=scale, uncond_cond=uc, prep=s.prepare(c, uncond_scale=scale, uncond_cond=uc)), want)
        # and that is the restatement on the same groups
        ref = rescale_ref.rescale(eg.cpu().numpy().reshape(groups, 2, -1), scales[0], scales[1] if groups == 3 else 0.0, PHI)
        assert (ulps_apart(wt.cpu().numpy(), ref["w"]) <= 1).all()
        assert np.array_equal(bits(got).reshape(2, -1), bits(rescale_ref.scale_rows(ref["e_cfg"], wt.cpu().numpy())))
        plain = SDFSampler(ldm, seed=3).get_eps(x, t, c, uncond_scale=scale, uncond_cond=uc)
        assert np.array_equal(bits(plain).reshape(2, -1), bits(ref["e_cfg"]))
    before = s.last_rescale
    assert torch.equal(s.get_eps(x, t, c, uncond_scale=1.0, uncond_cond=uc), ldm(x, t, c)) and s.last_rescale is before


@pytest.mark.parametrize("family", list(FAMILIES))
def test_a_captured_step_with_phi_is_the_eager_loop_and_is_keyed_by_phi(net, family):
    x, c, uc = inputs()

    def paint(s, scale):
        s._draws = 0                                                                # every run from the sampler's first draw (DDPM draws per step)
        return s.paint(x, c, 3, uncond_scale=scale, uncond_cond=uc)

    for scale in (SCALE,) + ((DualScale(3.0, 1.5, SPLIT),) if family == "ddim" else ()):
        eager = FAMILIES[family](LatentDiffusion(net), guidance_rescale=PHI).paint(x, c, 3, uncond_scale=scale, uncond_cond=uc)
        s = FAMILIES[family](LatentDiffusion(net), graph=True, guidance_rescale=PHI)
        assert torch.equal(paint(s, scale), eager) and s.graph_captures == 1
        s.guidance_rescale = 0.7                                                    # the same phi: the same capture
        assert torch.equal(paint(s, scale), eager) and s.graph_captures == 1
        s.guidance_rescale = 0.25
        other = paint(s, scale)
        assert s.graph_captures == 2 and not torch.equal(other, eager)
        assert torch.equal(other, FAMILIES[family](LatentDiffusion(net), guidance_rescale=0.25).paint(x, c, 3, uncond_scale=scale, uncond_cond=uc))
        s.guidance_rescale = 0.0
        assert torch.equal(paint(s, scale), FAMILIES[family](LatentDiffusion(net)).paint(x, c, 3, uncond_scale=scale, uncond_cond=uc))
    s.guidance_interval = (100, 200)
    with pytest.raises(ValueError, match="guidance_interval.*graph=True"):
        paint(s, SCALE)


class Counting:
    """A LatentDiffusion that notes the rows of x, t and the context of every denoiser call."""

    def __init__(self, ldm):
        self._ldm, self.calls = ldm, []

    def __getattr__(self, name):
        return getattr(self._ldm, name)

    def __call__(self, x, t, c, **kw):
        self.calls.append((x.shape[0], t.shape[0], c.shape[0]))
        return self._ldm(x, t, c, **kw)


def hand_loop(family, s, x, c, uc, taus, scale_at):
    """paint(x, c, 3) of `family` written out as p_sample calls, each with the scale `scale_at(time-step value)`."""
    x0p = None
    for index in range(3, -1, -1):
        tau = int(taus[index])
        kw = dict(uncond_scale=scale_at(tau), uncond_cond=uc)
        if family == "ddpm":
            x = s.p_sample(x, c, None, tau, return_x0=False, **kw)[0]
        elif family == "ddim":
            x = s.p_sample(x, c, None, tau, index, **kw)[0]
        else:
            x, x0p, _ = s.p_sample(x, c, None, tau, index, x0_prev=x0p, **kw)
    return x


@pytest.mark.parametrize("phi", [0.0, PHI])
@pytest.mark.parametrize("family", list(FAMILIES))
def test_an_interval_is_the_hand_written_loop_that_switches_the_scale(net, family, phi):
    x, c, uc = inputs()
    B = x.shape[0]
    taus = FAMILIES[family](LatentDiffusion(net)).time_steps[:4]                 # ddpm: 0..3; ddim: 1, 51, 101, 151; dpm: its logSNR grid
    lo, hi = int(taus[1]), int(taus[2])                                          # guided at the two middle steps only
    for scale, G in ((SCALE, 2), (DualScale(3.0, 1.5, SPLIT), 3)):
        cnt = Counting(LatentDiffusion(net))
        s = FAMILIES[family](cnt, guidance_rescale=phi, guidance_interval=(lo, hi))
        got = s.paint(x, c, 3, uncond_scale=scale, uncond_cond=uc)
        assert cnt.calls == [(B, B, B), (B, G * B, G * B), (B, G * B, G * B), (B, B, B)], cnt.calls
        hand = FAMILIES[family](LatentDiffusion(net), guidance_rescale=phi)
        want = hand_loop(family, hand, x, c, uc, taus, lambda tau: scale if lo <= tau <= hi else 1.0)
        assert torch.equal(got, want)
        always = FAMILIES[family](LatentDiffusion(net), guidance_rescale=phi)
        full = always.paint(x, c, 3, uncond_scale=scale, uncond_cond=uc)
        fresh = FAMILIES[family](LatentDiffusion(net), guidance_rescale=phi)
        assert not torch.equal(got, full) and torch.equal(full, hand_loop(family, fresh, x, c, uc, taus, lambda tau: scale))
        # p_sample on its own resolves the interval too, and get_eps does when it is told the time step
        lone = FAMILIES[family](LatentDiffusion(net), guidance_rescale=phi, guidance_interval=(lo, hi))
        assert torch.equal(hand_loop(family, lone, x, c, uc, taus, lambda tau: scale), got)
    t = torch.full((B,), int(taus[3]), dtype=torch.long, device="cuda")
    assert torch.equal(lone.get_eps(x, t, c, uncond_scale=SCALE, uncond_cond=uc, t_value=int(taus[3])), LatentDiffusion(net)(x, t, c))
    with pytest.raises(ValueError, match="t_value"):
        lone.get_eps(x, t, c, uncond_scale=SCALE, uncond_cond=uc)


def test_invert_and_morph_resolve_the_interval(net):
    x, c, uc = inputs()
    taus = DDIMSampler(LatentDiffusion(net), 20, "uniform", 0.0).time_steps[:4]
    cnt = Counting(LatentDiffusion(net))
    s = DDIMSampler(cnt, 20, "uniform", 0.0, seed=3, guidance_rescale=PHI, guidance_interval=(int(taus[1]), int(taus[2])))
    up = s.invert(x, c, 3, iters=2, uncond_scale=SCALE, uncond_cond=uc)
    B = x.shape[0]
    assert cnt.calls == [(B, B, B)] * 2 + [(B, 2 * B, 2 * B)] * 4 + [(B, B, B)] * 2 and torch.isfinite(up).all()
    cnt.calls.clear()
    frames = s.morph(x[:1], c[:1], x[1:], c[1:], 3, t_end=3, iters=1, uncond_scale=SCALE, uncond_cond=uc[:1])
    assert frames.shape == (3, 1, 2, 32, 32) and torch.isfinite(frames).all()
    assert cnt.calls == [(2, 2, 2), (2, 4, 4), (2, 4, 4), (2, 2, 2)] + [(3, 3, 3), (3, 6, 6), (3, 6, 6), (3, 3, 3)]


def test_under_a_window_plan_the_rescale_runs_on_the_windows_and_the_merge_is_plain(lib, net):
    wp = WindowPlan(2, 16, 32)
    x, c, uc = inputs(1, wp.canvas_h)[0], inputs(2)[1], inputs(2)[2]            # one song of two windows: a canvas, and one condition row per window
    ldm = LatentDiffusion(net)
    s = DDIMSampler(ldm, 20, "uniform", 0.0, seed=3, windows=wp, guidance_rescale=PHI)
    t = torch.tensor([500, 500]).cuda()
    xw = _steps.window_split(lib, x, wp.n_windows, wp.stride, wp.win_h)
    eg = ldm(xw, torch.cat([t, t]), torch.cat([uc, c]), shared_x=True).clone()
    ew, st, wt = _steps.cfg_rescale(lib, eg, 2, (SCALE,), PHI, want_stats=True)
    want = _steps.window_merge(lib, ew, s._window_weights(wp, x.device), 1, wp.n_windows, wp.stride, 1, ())
    got = s.get_eps(x, t, c, uncond_scale=SCALE, uncond_cond=uc)
    assert got.shape == (1, 2, wp.canvas_h, 32) and torch.equal(got, want)
    assert s.last_rescale[1].shape == (2,) and torch.equal(s.last_rescale[1], wt)      # one weight per WINDOW
    s.guidance_rescale = 0.0
    assert torch.equal(s.get_eps(x, t, c, uncond_scale=SCALE, uncond_cond=uc),
                       _steps.window_merge(lib, eg, s._window_weights(wp, x.device), 1, wp.n_windows, wp.stride, 2, (SCALE,)))
    # a loop with both settings on the canvas: eager, finite, and not the plain one
    s.guidance_rescale, s.guidance_interval = PHI, (51, 101)
    out = s.paint(x, c, 3, uncond_scale=SCALE, uncond_cond=uc)
    assert torch.isfinite(out).all() and not torch.equal(out, DDIMSampler(ldm, 20, "uniform", 0.0, seed=3, windows=wp).paint(x, c, 3, uncond_scale=SCALE, uncond_cond=uc))


# ---------------------------------------------------------------------------------------------- the CLI
def test_cli_writes_a_stamp_that_names_both_settings_and_repeats_under_a_seed(tmp_path):
    from polyffusion_amd import inference_sdf
    runs = []
    for name in ("a", "b"):
        out = tmp_path / name
        argv = ["--params_preset", "sdf_chd8bar", "--synthetic_weights", "--synthetic", "--length", "1", "--dpm", "--dpm_steps", "4",
                "--uncond_scale", "3", "--guidance_rescale", "0.7", "--guidance_interval", "0.2", "0.8", "--seed", "7", "--output_dir", str(out)]
        assert inference_sdf.main(argv) == 0
        mids = [f for f in os.listdir(out) if f.endswith(".mid")]
        npys = [f for f in os.listdir(out) if f.endswith(".npy")]
        assert len(mids) == 1 and len(npys) == 1 and os.path.getsize(out / mids[0]) > 0
        assert "[scale=3.0,rescale=0.7,interval=200-799]" in mids[0] and mids[0].startswith("sdf_chd8bar")
        runs.append(np.load(out / npys[0]))
    assert np.isfinite(runs[0]).all() and runs[0].shape == (1, 2, 128, 128)
    assert np.array_equal(runs[0].view(np.uint32), runs[1].view(np.uint32))
