"""Exact DDIM inversion on the GPU (-m gpu): ``pf_invert_step`` against the float64 restatement in ``tests/invert_ref.py`` on every route
(coefficients by value and from a device table, the previous iterate aliased / separate / absent, with and without the fused residual,
16-byte vector and scalar path, one and several rows and chunks), what it must not touch, its residual sums against float64 sums of its
own output and their independence of how the batch is split; ``DDIMSampler.invert`` on the closed-form Gaussian denoiser - rounding
against the float64 loop and the float64 round trip - and on a small synthetic UNet (eager == captured graph, repeatable, a lower depth,
the per-step identity between the forward step's defect and the next residual, window plans, dual guidance), and the CLI.

Error budgets (``invert_ref.budget`` / ``forward_budget``): the roundings counted beside the kernels times 2^-24 times the magnitudes of
the terms they act on; inputs are O(1), so nothing is subnormal.  No test asserts a convergence rate or a round-trip size on a UNet."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import dpm_ref  # noqa: E402
import invert_ref  # noqa: E402
from polyffusion_amd import _lib, _steps  # noqa: E402
from polyffusion_amd.arch import UNetConfig  # noqa: E402
from polyffusion_amd.sampler import DDIMSampler, DualScale, WindowPlan  # noqa: E402

T = 5                   # the small-UNet loops: 6 steps, grid indices 0 .. 5 (the CLI's t_idx = ddim_steps - 1)
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
AB = dpm_ref.alpha_bar()
ROWS = invert_ref.rows(AB, dpm_ref.grid_uniform(1000, 10)).astype(np.float32)          # the shipped schedule's 10-step rows, as the kernel gets them
ROW = ROWS[5]
CHUNK = _lib.MSE_CHUNK
NS = [1, 4, 7, 1024, 1027, 2 * CHUNK + 5]
PAD = 8                 # elements of sentinel on either side of an output (floats: 32 bytes, the payload keeps its 16-byte alignment)
SENTINEL = -777.25
N_SLOTS, ITERS, K_IT, SLOT = 8, 3, 1, 7        # residual table of 8 slots; state {index 2} with iters 3, k 1 names slot 7, as does slot = 7 by value
U53 = 2.0 ** -53


@pytest.fixture(scope="module")
def lib():
    _lib.require_gpu()
    return _lib.load()


@pytest.fixture(scope="module")
def data():
    """name -> float32 numpy array of 3 rows of the largest size (read-only: every test copies what it needs to the device)."""
    g = torch.Generator().manual_seed(17)
    d = {k: torch.randn(3 * (2 * CHUNK + 8), generator=g).numpy() for k in ("y", "eps", "xi")}
    for v in d.values():
        v.setflags(write=False)
    return d


def padded(values, off=0, dtype=torch.float32):
    """(whole buffer, payload view) on the device: the payload starts `off` elements past a 16-byte boundary, sentinels around it."""
    n = len(values)
    whole = torch.full((n + 2 * PAD + 4,), SENTINEL, device="cuda", dtype=dtype)
    view = whole[PAD + off: PAD + off + n]
    view.copy_(torch.from_numpy(np.array(values, dtype=np.float32 if dtype == torch.float32 else np.float64)))
    return whole, view


def untouched(whole, view_len, off=0):
    w = whole.cpu().numpy()
    return (w[: PAD + off] == SENTINEL).all() and (w[PAD + off + view_len:] == SENTINEL).all()


def sources(lib):
    """The two coefficient sources: a host struct, and row 2 of a four-row device table with state = {index 2}; the other rows differ."""
    table = torch.from_numpy(np.stack([ROWS[1], ROWS[7], ROW, ROWS[3]])).cuda()
    state = torch.zeros(2, dtype=torch.int64, device="cuda")
    _lib.check(lib.pf_step_state_set(state.data_ptr(), 2, 0, _lib.current_stream()), "pf_step_state_set")
    return dict(coef=_lib.InvertCoef(float(ROW[0]), float(ROW[1]))), dict(table=table, state=state)


def run(lib, h, rows, n, off, xi_mode, src, with_resid):
    """One launch on rows x n elements of the host data `h` (a dict of flat float32 arrays holding at least rows * n elements); returns
    (x_out [rows, n], resid [rows, 2] or None) as numpy after checking the sentinels and that the inputs are unchanged.
    xi_mode: "alias" (x_out is x_iter) | "separate" | "null"."""
    tot = rows * n
    dev = {k: padded(h[k][:tot], off) for k in ("y", "eps", "xi")}
    out_w, out = dev["xi"] if xi_mode == "alias" else padded(np.zeros(tot, np.float32), off)
    xi = None if xi_mode == "null" else dev["xi"][1]
    kw = {}
    if with_resid:
        res_w, res = padded(np.full(N_SLOTS * rows * 2, SENTINEL), 0, torch.float64)
        nb = int(lib.pf_invert_step_workspace_bytes(rows, n))
        ws_w, ws = padded(np.full(nb // 8, SENTINEL), 0, torch.float64)
        kw = dict(resid=res.view(N_SLOTS, rows, 2), workspace=ws, iters=ITERS, k=K_IT, slot=SLOT)
    _steps.invert_step(lib, dev["y"][1].view(rows, n), dev["eps"][1].view(rows, n), out.view(rows, n), x_iter=None if xi is None else xi.view(rows, n),
                       **kw, **src)
    torch.cuda.synchronize()
    assert untouched(out_w, tot, off)
    for k in ("y", "eps") + (("xi",) if xi_mode == "separate" else ()):       # inputs are read-only, unless they are the aliased output
        assert np.array_equal(dev[k][1].cpu().numpy(), h[k][:tot]) and untouched(dev[k][0], tot, off)
    r = None
    if with_resid:
        assert untouched(res_w, N_SLOTS * rows * 2) and untouched(ws_w, nb // 8)
        table = res.cpu().numpy().reshape(N_SLOTS, rows, 2)
        assert (np.delete(table, SLOT, axis=0) == SENTINEL).all()            # the other slots of the table stay as they were
        r = table[SLOT]
    return out.cpu().numpy().reshape(rows, n), r


def host_sums(out, prev):
    """Per row: (exactly summed float64 terms of (out - prev)^2 with the difference in float32, the same for out^2)."""
    d = (out - prev).astype(np.float64)                                      # float32 subtraction, as the kernel's sub_rn
    return np.array([[math.fsum(d[b] ** 2), math.fsum(out[b].astype(np.float64) ** 2)] for b in range(out.shape[0])])


# ---------------------------------------------------------------------------------------------- the kernel
@pytest.mark.parametrize("rows", [1, 3])
@pytest.mark.parametrize("n", NS)
def test_one_iterate_on_every_route(lib, data, n, rows):
    off = 1 if n == 1027 else 0                                              # this size from a base 4 bytes past a 16-byte boundary
    tot = rows * n
    y, eps, xi = (data[k][:tot].reshape(rows, n) for k in ("y", "eps", "xi"))
    want, bud = invert_ref.update(ROW, y, eps), invert_ref.budget(ROW, y, eps)
    outs, resids = [], {"xi": [], "null": []}
    for xi_mode in ("alias", "separate", "null"):
        for si, src in enumerate(sources(lib)):
            for with_resid in (True, False):
                got, r = run(lib, data, rows, n, off, xi_mode, src, with_resid)
                err = np.abs(got - want)
                print(f"n={n} rows={rows} xi={xi_mode} src={si} resid={with_resid}: max err/budget {np.max(err / bud):.3f}")
                assert (err <= bud).all(), (xi_mode, si, with_resid, float(np.max(err / bud)))
                outs.append(got)
                if r is not None:
                    resids["null" if xi_mode == "null" else "xi"].append(r)
                    # against float64 sums of the kernel's OWN float32 output: n terms added in some order, each sum rounded once
                    ref = host_sums(got, y if xi_mode == "null" else xi)
                    assert (np.abs(r - ref) <= n * U53 * ref).all(), (xi_mode, si, r, ref)
    assert all(np.array_equal(o.view(np.uint32), outs[0].view(np.uint32)) for o in outs)           # every route computes the same bits
    for rs in resids.values():
        assert len(rs) >= 2 and all(np.array_equal(r.view(np.uint64), rs[0].view(np.uint64)) for r in rs)


@pytest.mark.parametrize("n", NS)
def test_residual_of_a_row_does_not_depend_on_how_the_batch_is_split(lib, data, n):
    off = 1 if n == 1027 else 0
    src = sources(lib)[0]
    for xi_mode in ("separate", "null"):
        out3, r3 = run(lib, data, 3, n, off, xi_mode, src, True)
        for b in range(3):
            hb = {k: v[b * n:] for k, v in data.items()}
            out1, r1 = run(lib, hb, 1, n, off, xi_mode, src, True)
            assert np.array_equal(out1[0].view(np.uint32), out3[b].view(np.uint32))
            assert np.array_equal(r1[0].view(np.uint64), r3[b].view(np.uint64)), (xi_mode, b)


def test_vector_and_scalar_paths_give_the_same_bits(lib, data):
    src = sources(lib)[0]
    for n in (1024, 2 * CHUNK + 8):
        for with_resid in (True, False):
            a, ra = run(lib, data, 3, n, 0, "separate", src, with_resid)     # every tensor 16-byte aligned, n % 4 == 0: vectors
            b, rb = run(lib, data, 3, n, 1, "separate", src, with_resid)     # the same values 4 bytes further on: element by element
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
            assert ra is None or np.array_equal(ra.view(np.uint64), rb.view(np.uint64))


def test_step_advance_moves_the_state_and_the_slot_follows_it(lib, data):
    state = torch.zeros(2, dtype=torch.int64, device="cuda")
    _lib.check(lib.pf_step_state_set(state.data_ptr(), 1, 5, _lib.current_stream()), "pf_step_state_set")
    _lib.check(lib.pf_step_advance(state.data_ptr(), 1, 2, _lib.current_stream()), "pf_step_advance")
    assert state.cpu().tolist() == [2, 7]
    table = torch.from_numpy(np.stack([ROWS[1], ROWS[7], ROW, ROWS[3]])).cuda()
    n = 64
    y, eps = (torch.from_numpy(data[k][:n].copy()).cuda().view(1, n) for k in ("y", "eps"))
    resid = torch.full((4 * 2, 1, 2), SENTINEL, dtype=torch.float64, device="cuda")
    ws = _steps.invert_workspace(lib, 1, n, "cuda")
    out = _steps.invert_step(lib, y, eps, torch.empty_like(y), table=table, state=state, resid=resid, workspace=ws, iters=2, k=1)
    r = resid.cpu().numpy()
    assert (np.delete(r, 5, axis=0) == SENTINEL).all() and (r[5] != SENTINEL).all()      # slot = index 2 * iters 2 + k 1
    assert (np.abs(out.cpu().numpy() - invert_ref.update(ROW, data["y"][:n], data["eps"][:n])) <= invert_ref.budget(ROW, data["y"][:n], data["eps"][:n])).all()
    # a slot the table does not have is left unwritten by the device-side guard (memory safety only)
    _lib.check(lib.pf_step_advance(state.data_ptr(), 1, 0, _lib.current_stream()), "pf_step_advance")
    before = resid.clone()
    _steps.invert_step(lib, y, eps, torch.empty_like(y), table=table, state=state, resid=resid[:6], workspace=ws, iters=2, k=1)   # slot 7 of 6
    assert torch.equal(resid, before)


# ---------------------------------------------------------------------------------------------- the loop on the analytic denoiser
class GaussianDenoiser:
    """Stands in for a LatentDiffusion: the optimal denoiser of data ~ N(0, s^2), eps = gain[t] * x as ONE float32 product on the device.
    Carries what the samplers touch: n_steps, alpha_bar, and an eps_model with the two prepare hooks."""

    def __init__(self, s):
        self.n_steps = 1000
        self.alpha_bar = torch.from_numpy(AB.astype(np.float32))
        self.eps_model = self
        self.gain32 = dpm_ref.gauss_gain(AB, np.arange(1000), s).astype(np.float32)
        self.gain = torch.from_numpy(self.gain32).cuda()

    def prepare_time(self, n, out=None):
        return None

    def prepare_cond(self, ctx, out=None):
        return None

    def __call__(self, x, t, c, time_table=None, cross_bias=None):
        return x * self.gain[t].view(-1, 1, 1, 1)


@pytest.fixture(scope="module")
def x_0():
    return torch.randn(2, 2, 8, 8, generator=torch.Generator().manual_seed(5))


def ddim_rows_of(sd):
    """The sampler's own float32 DDIM coefficients (s1m, sqrt_a, sqrt_aprev, dir_coef) per index, as float64."""
    return np.array([[getattr(sd._coef(i), f) for f in ("s1m", "sqrt_a", "sqrt_aprev", "dir_coef")] for i in range(len(sd.time_steps))], dtype=np.float64)


@pytest.fixture(scope="module")
def gauss_runs(lib, x_0):
    """(s, steps, K) -> (inverted x, its repaint, residuals(), the kept iterates, the table, sampler, model): every loop run once."""
    cond = torch.zeros(2, 1, 4, device="cuda")
    out = {}
    for s in (0.5, 1.0, 4.0):
        m = GaussianDenoiser(s)
        for n in (50, 10):
            sd = DDIMSampler(m, n, "uniform", 0.0)
            t = len(sd.time_steps) - 1
            for K in (1, 3, 8):
                x = sd.invert(x_0.cuda(), cond, iters=K, keep_iterates=True)
                rec = sd.last_inversion
                back = sd.paint(x, cond, t)
                its = [[v.cpu().numpy() for v in step] for step in rec.iterates]
                out[(s, n, K)] = (x.cpu().numpy(), back.cpu().numpy(), rec.residuals(), its, rec.table.cpu().numpy(), sd, m)
    return out


CASES = [(s, n, K) for s in (0.5, 1.0, 4.0) for n in (50, 10) for K in (1, 3, 8)]


@pytest.mark.parametrize("s,n,K", CASES)
def test_invert_stays_within_the_accumulated_budget_of_the_float64_loop(gauss_runs, x_0, s, n, K):
    got, _, _, _, _, sd, m = gauss_runs[(s, n, K)]
    assert len(sd.time_steps) == n
    want, bound, _ = invert_ref.invert_gauss_with_budget(sd.invert_rows().astype(np.float64), m.gain32[sd.time_steps].astype(np.float64), x_0.numpy(), K)
    err = np.abs(got - want)
    print(f"s={s} n={n} K={K}: max err {err.max():.3e}, max err/bound {np.max(err / bound):.3f}")
    assert (err <= bound).all(), float(np.max(err / bound))


@pytest.mark.parametrize("s,n,K", CASES)
def test_paint_of_invert_stays_within_the_bound_of_the_float64_round_trip(gauss_runs, x_0, s, n, K):
    _, got, _, _, _, sd, m = gauss_runs[(s, n, K)]
    gains = m.gain32[sd.time_steps].astype(np.float64)
    x, bound, _ = invert_ref.invert_gauss_with_budget(sd.invert_rows().astype(np.float64), gains, x_0.numpy(), K)
    want, bound = invert_ref.paint_gauss_with_budget(ddim_rows_of(sd), gains, x, bound)
    err = np.abs(got - want)
    print(f"s={s} n={n} K={K}: max err {err.max():.3e}, max err/bound {np.max(err / bound):.3f}; round trip of the float64 loop "
          f"{np.abs(want - x_0.numpy()).max():.3e}, of the float32 one {np.abs(got - x_0.numpy()).max():.3e}")
    assert (err <= bound).all(), float(np.max(err / bound))


@pytest.mark.parametrize("s,n,K", CASES)
def test_residuals_are_the_sums_over_the_kept_iterates(gauss_runs, x_0, s, n, K):
    _, _, res, its, table, sd, _ = gauss_runs[(s, n, K)]
    assert res.shape == (n, K, 2) and table.shape == (n, K, 2, 2) and len(its) == n and all(len(v) == K for v in its)
    y, elems = x_0.numpy(), x_0[0].numel()
    for i in range(n):
        for k in range(K):
            prev = y if k == 0 else its[i][k - 1]
            ref = host_sums(its[i][k].reshape(2, -1), prev.reshape(2, -1))
            assert (np.abs(table[i, k] - ref) <= elems * U53 * ref).all(), (i, k)
            # residuals() is sqrt(sum diff^2 / sum x^2) of the table: two sums within elems * 2^-53 each, a division and a square root
            want = np.sqrt(ref[:, 0] / ref[:, 1])
            assert (np.abs(res[i, k] - want) <= (elems + 2) * U53 * want).all(), (i, k)
        y = its[i][-1]


# ---------------------------------------------------------------------------------------------- a small synthetic UNet
@pytest.fixture(scope="module")
def ldm():
    from polyffusion_amd.unet import LatentDiffusion, UNetModel
    from polyffusion_amd.weights import synth_unet_state
    kw = dict(in_channels=2, out_channels=2, channels=32, n_res_blocks=1, attention_levels=(1,), channel_multipliers=(1, 2), n_heads=2,
              tf_layers=1, d_cond=32)
    m = UNetModel(img_h=16, img_w=16, **kw)
    m.load_state_dict(synth_unet_state(UNetConfig(**kw), 0))
    m.set_precision("bf16x3")
    return LatentDiffusion(m, None, 0.18215, 1000, 0.00085, 0.012)


def unet_inputs():
    g = torch.Generator().manual_seed(3)
    x, cond = (torch.randn(*s, generator=g).cuda() for s in ((2, 2, 16, 16), (2, 1, 32)))
    return x, cond


def guidance(scale, rows=2):
    return dict(uncond_scale=scale, uncond_cond=-torch.ones(rows, 1, 32).cuda())


@pytest.mark.parametrize("scale", [1.0, 5.0])
def test_invert_eager_graph_repeat_and_depth(ldm, scale):
    x0, cond = unet_inputs()
    kw = dict(iters=2, **guidance(scale))
    eager = DDIMSampler(ldm, 6, "uniform", 0.0)
    assert len(eager.time_steps) == 7                                        # 'uniform' at 6 yields one more entry: 6 steps = indices 0 .. 5
    a = eager.invert(x0.clone(), cond, T, **kw)
    ta = eager.last_inversion.table.clone()
    assert torch.isfinite(a).all() and eager.last_inversion.shape == (6, 2, 2, 2) and not torch.equal(a, x0)
    other = eager.invert(-x0, cond, T, **kw)
    assert not torch.equal(a, other)
    assert torch.equal(eager.invert(x0.clone(), cond, T, **kw), a) and torch.equal(eager.last_inversion.table, ta)      # a repeated call: same bits
    assert torch.equal(DDIMSampler(ldm, 6, "uniform", 0.0).invert(x0.clone(), cond, T, **kw), a)
    graph = DDIMSampler(ldm, 6, "uniform", 0.0, graph=True)
    b = graph.invert(x0.clone(), cond, T, **kw)
    assert graph.graph_captures == 1 and torch.equal(a, b)
    assert graph.last_inversion.shape == (6, 2, 2, 2) and torch.equal(graph.last_inversion.table, ta)
    assert torch.equal(graph.invert(-x0, cond, T, **kw), other)
    assert torch.equal(graph.invert(x0.clone(), cond, T, **kw), a) and graph.graph_captures == 1
    assert np.isfinite(graph.last_inversion.residuals()).all()
    # a depth below the top: the first depth + 1 steps of the full walk, the level paint(t_start = depth) starts from
    eager.invert(x0.clone(), cond, T, keep_iterates=True, **kw)
    at3 = eager.last_inversion.iterates[3][-1]
    low = eager.invert(x0.clone(), cond, 3, **kw)
    assert torch.equal(low, at3) and eager.last_inversion.shape == (4, 2, 2, 2) and torch.equal(eager.last_inversion.table, ta[:4])
    assert torch.equal(graph.invert(x0.clone(), cond, 3, **kw), low) and graph.graph_captures == 1
    assert torch.equal(graph.last_inversion.table, ta[:4])
    back = eager.paint(low, cond, 3, **guidance(scale))
    assert torch.isfinite(back).all() and back.shape == x0.shape
    print(f"scale={scale}: last-iterate residuals {eager.last_inversion.residuals()[:, -1].max():.3e}, "
          f"round trip from depth 3 max |x - x_rec| {(back - x0).abs().max().item():.3e} (printed, not asserted)")


@pytest.mark.parametrize("scale", [1.0, 5.0])
def test_forward_step_defect_is_the_next_residual_over_c_y(ldm, lib, scale):
    """One step of the loop: F(x_K) - y = (x_K - x_K+1) / c_y, with F the pf_ddim_step on x_K.  Exact in exact arithmetic with exact
    coefficients; the bound counts the roundings of the two kernels on the same eps (forward_budget, budget / c_y), the one float32
    difference x_K - x_K+1, and what the two kernels' float32 coefficients - formed separately - differ by as functions."""
    x0, cond = unet_inputs()
    K, i = 2, 3
    sd = DDIMSampler(ldm, 6, "uniform", 0.0)
    g = guidance(scale)
    sd.invert(x0.clone(), cond, T, iters=K, keep_iterates=True, **g)
    its = sd.last_inversion.iterates
    y, x_K = its[i - 1][-1], its[i][K - 1]
    prep = sd.prepare(cond, **g)
    e = sd._eps(x_K, cond, int(sd.time_steps[i]), g["uncond_scale"], g["uncond_cond"], None, prep).contiguous()
    R, D = sd.invert_rows()[i].astype(np.float64), ddim_rows_of(sd)[i]
    x_K1 = _steps.invert_step(lib, y, e, torch.empty_like(y), coef=_lib.InvertCoef(float(R[0]), float(R[1])), x_iter=x_K)
    fx = _steps.ddim_step(lib, x_K, e, torch.empty_like(x_K), coef=sd._coef(i))
    y64, xk, xk1, e64, fx64 = (v.cpu().numpy().astype(np.float64) for v in (y, x_K, x_K1, e, fx))
    lhs = fx64 - y64
    rhs = (x_K - x_K1).cpu().numpy().astype(np.float64) / R[0]               # the difference in float32, as the residual forms it
    s1m, sqrt_a, sqrt_ap, dirc = D
    coef_gap = abs(sqrt_ap / sqrt_a - 1 / R[0]) * np.abs(xk) + abs((dirc - sqrt_ap * s1m / sqrt_a) + R[1] / R[0]) * np.abs(e64)
    bound = (invert_ref.forward_budget(D, xk, e64) + invert_ref.budget(R, y64, e64) / R[0] + invert_ref.U * np.abs(xk - xk1) / R[0] + coef_gap)
    err = np.abs(lhs - rhs)
    print(f"scale={scale}: defect max {np.abs(lhs).max():.3e}, |lhs - rhs| max {err.max():.3e}, max err/bound {np.max(err / bound):.3f}, "
          f"coefficient part of the bound {np.max(coef_gap / bound):.2f}")
    assert (err <= bound).all(), float(np.max(err / bound))


def test_window_plans_and_dual_guidance(ldm):
    x0, cond = unet_inputs()
    kw = dict(iters=2, **guidance(5.0))
    plain = DDIMSampler(ldm, 6, "uniform", 0.0)
    a = plain.invert(x0.clone(), cond, T, **kw)
    ta = plain.last_inversion.table.clone()
    one = DDIMSampler(ldm, 6, "uniform", 0.0, windows=WindowPlan(1, 8, 16))  # every image a canvas of one window
    assert torch.equal(one.invert(x0.clone(), cond, T, **kw), a) and torch.equal(one.last_inversion.table, ta)
    plan = WindowPlan(3, 8, 16)                                              # a two-segment canvas: three half-overlapping windows
    canvas = torch.cat([x0[0], x0[1]], dim=1).unsqueeze(0).contiguous()
    assert canvas.shape == (1, 2, plan.canvas_h, 16)
    cw = torch.cat([cond, cond[:1]]).contiguous()
    for graph in (False, True):
        sw = DDIMSampler(ldm, 6, "uniform", 0.0, windows=plan, graph=graph)
        out = sw.invert(canvas, cw, T, iters=2, **guidance(5.0, 3))
        assert out.shape == canvas.shape and torch.isfinite(out).all() and sw.last_inversion.shape == (6, 2, 1, 2)
        assert np.isfinite(sw.last_inversion.residuals()).all()
        if graph:
            assert torch.equal(out, first)
        first = out
    dual = DDIMSampler(ldm, 6, "uniform", 0.0)
    d = dual.invert(x0.clone(), cond, T, iters=2, uncond_scale=DualScale(5.0, 5.0, 16), uncond_cond=kw["uncond_cond"])
    assert torch.equal(d, a) and torch.equal(dual.last_inversion.table, ta)
    d2 = dual.invert(x0.clone(), cond, T, iters=2, uncond_scale=DualScale(5.0, 2.0, 16), uncond_cond=kw["uncond_cond"])
    assert torch.isfinite(d2).all() and not torch.equal(d2, a)


# ---------------------------------------------------------------------------------------------- the CLI
def run_cli(tmp_path, shift):
    from polyffusion_amd import synth
    rng = np.random.default_rng(4)
    song = tmp_path / "song.npz"
    np.savez(song, chord=synth.chords(1, 104).astype(np.float32), prmat2c=(rng.random((1, 2, 128, 128)) > 0.97).astype(np.float32))
    out = tmp_path / f"out{shift}"
    cmd = [sys.executable, "-m", "polyffusion_amd.inference_sdf", "--params_preset", "sdf_chd8bar", "--synthetic_weights", "--cond_npz", str(song),
           "--ddim", "--ddim_steps", "4", "--edit", "--edit_iters", "2", "--edit_chord_shift", str(shift), "--edit_roundtrip", "--seed", "9",
           "--output_dir", str(out)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300, env=dict(os.environ, PYTHONPATH=REPO), cwd=REPO)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return out, r.stdout


def test_cli_writes_its_midi_file_and_reports_the_inversion(tmp_path):
    out, said = run_cli(tmp_path, 2)
    names = os.listdir(out)
    mids = [f for f in names if f.endswith(".mid")]
    npys = [f for f in names if f.endswith(".npy") and not f.endswith("_roundtrip.npy")]
    assert len(mids) == 1 and os.path.getsize(out / mids[0]) > 0 and len(npys) == 1 and "_edit2" in mids[0] and "_edit2" in npys[0]
    gen = np.load(out / npys[0])
    assert gen.shape == (1, 2, 128, 128) and np.isfinite(gen).all()
    assert "largest relative residual of the last iterate over all steps" in said
    assert "max |x - x_rec|" in said and "note cells > 0.5 that differ" in said
    assert not np.array_equal(gen, np.load(out / npys[0].replace(".npy", "_roundtrip.npy")))       # other chords: another song


def test_cli_with_no_shift_the_edit_is_its_own_round_trip(tmp_path):
    out, _ = run_cli(tmp_path, 0)
    npys = sorted(f for f in os.listdir(out) if f.endswith(".npy"))
    assert len(npys) == 2 and npys[1].endswith("_roundtrip.npy")
    a, b = np.load(out / npys[0]), np.load(out / npys[1])
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
