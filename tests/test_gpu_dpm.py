"""DPM-Solver++(2M) on the GPU (-m gpu): ``pf_dpm_step`` against the float64 restatement in ``tests/dpm_ref.py`` on every route (first and
second order, known region, the two aliasings, no x0 output, coefficients by value and from a device table, 16-byte vector and scalar
path), what it must not touch or read, ``DPMSolverSampler``'s loop on the closed-form Gaussian denoiser - rounding against the float64
loop, solver error against the exact ODE solution - and on a small synthetic UNet (eager == captured graph, repeatable, no history
carried between calls, a grid that repeats time steps), and the CLI.

Error budgets (``dpm_ref.budget``): the roundings counted beside the kernel times 2^-24 times the sum of the term magnitudes; inputs are
O(1), so nothing is subnormal."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import dpm_ref  # noqa: E402
from polyffusion_amd import _lib, _steps  # noqa: E402
from polyffusion_amd.arch import UNetConfig  # noqa: E402
from polyffusion_amd.sampler import DDIMSampler, DPMSolverSampler  # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
AB = dpm_ref.alpha_bar()
ROWS = dpm_ref.rows(AB, dpm_ref.grid_logsnr(AB, 10)).astype(np.float32)      # the shipped schedule's 10-step rows, as the kernel gets them
FIRST, SECOND = ROWS[9], ROWS[5]
assert FIRST[4] == 0 and SECOND[4] != 0
NS = [1, 4, 7, 1024, 1027]
PAD = 8                 # floats of sentinel on either side of an output (32 bytes: the payload keeps its 16-byte alignment)
SENTINEL = -777.25
NAMES = ("x", "eps", "x0_prev", "orig", "orig_noise", "mask")


@pytest.fixture(scope="module")
def lib():
    _lib.require_gpu()
    return _lib.load()


@pytest.fixture(scope="module")
def data():
    """name -> float32 numpy array of 1028 elements (read-only: every test copies what it needs to the device)."""
    g = torch.Generator().manual_seed(11)
    d = {k: torch.randn(1028, generator=g).numpy() for k in NAMES[:5]}
    m = (torch.rand(1028, generator=g) > 0.3).float()
    m[::7] = 0.25                                                            # a few soft mask values: the blend's products then round
    d["mask"] = m.numpy()
    for v in d.values():
        v.setflags(write=False)
    return d


def padded(values, off=0):
    """(whole buffer, payload view) on the device: the payload starts `off` floats past a 16-byte boundary, sentinels around it."""
    n = len(values)
    whole = torch.full((n + 2 * PAD + 4,), SENTINEL, device="cuda")
    view = whole[PAD + off: PAD + off + n]
    view.copy_(torch.from_numpy(np.array(values, dtype=np.float32)))
    return whole, view


def untouched(whole, view_len, off=0):
    w = whole.cpu().numpy()
    return (w[: PAD + off] == SENTINEL).all() and (w[PAD + off + view_len:] == SENTINEL).all()


def sources(lib, row):
    """The two coefficient sources: a host struct, and row 2 of a four-row device table with state = {index 2}; the other rows differ."""
    table = torch.from_numpy(np.stack([ROWS[1], ROWS[7], row, ROWS[3]])).cuda()
    state = torch.zeros(2, dtype=torch.int64, device="cuda")
    _lib.check(lib.pf_step_state_set(state.data_ptr(), 2, 0, _lib.current_stream()), "pf_step_state_set")
    return dict(coef=_lib.DpmCoef(*(float(v) for v in row))), dict(table=table, state=state)


def bits(t):
    return t.cpu().numpy().view(np.uint32)


def run(lib, row, h, n, off, known, alias, src):
    """One launch on the leading n elements of the host data `h`; returns (x_out, x0 or None) as numpy after checking the sentinels.
    alias: "none" | "x" (x_out is x) | "x0" (x0_out is x0_prev) | "nox0" (x0_out NULL)."""
    dev = {k: padded(h[k][:n], off) for k in NAMES}
    out_w, out = dev["x"] if alias == "x" else padded(np.zeros(n, np.float32), off)
    if alias == "nox0":
        x0_w, x0 = None, None
    else:
        x0_w, x0 = dev["x0_prev"] if alias == "x0" else padded(np.zeros(n, np.float32), off)
    kw = dict(orig=dev["orig"][1], orig_noise=dev["orig_noise"][1], mask=dev["mask"][1]) if known else {}
    _steps.dpm_step(lib, dev["x"][1], dev["eps"][1], out, x0_prev=dev["x0_prev"][1], x0_out=x0, **kw, **src)
    torch.cuda.synchronize()
    assert untouched(out_w, n, off) and (x0_w is None or untouched(x0_w, n, off))
    for k in NAMES:                                                          # inputs are read-only, unless they are an aliased output
        if not (k == "x" and alias == "x") and not (k == "x0_prev" and alias == "x0"):
            assert np.array_equal(dev[k][1].cpu().numpy(), h[k][:n]) and untouched(dev[k][0], n, off)
    return out.cpu().numpy(), None if x0 is None else x0.cpu().numpy()


# ---------------------------------------------------------------------------------------------- one update
@pytest.mark.parametrize("n", NS)
def test_one_update_is_within_its_rounding_budget_of_float64(lib, data, n):
    off = 1 if n == 1027 else 0                                              # the last size from a base 4 bytes past a 16-byte boundary
    results = {}
    for order, row in (("first", FIRST), ("second", SECOND)):
        for known in (False, True):
            kn = {k: data[k][:n] for k in ("orig", "orig_noise", "mask")} if known else {}
            want, want0 = dpm_ref.update(row, data["x"][:n], data["eps"][:n], data["x0_prev"][:n], **kn)
            bx, b0 = dpm_ref.budget(row, data["x"][:n], data["eps"][:n], data["x0_prev"][:n], **kn)
            for alias in ("none", "x", "x0", "nox0"):
                for si, src in enumerate(sources(lib, row)):
                    got, got0 = run(lib, row, data, n, off, known, alias, src)
                    ex = np.abs(got - want)
                    print(f"n={n} {order} known={known} alias={alias} src={si}: max err/budget {np.max(ex / bx):.3f}")
                    assert (ex <= bx).all(), (order, known, alias, si, float(np.max(ex / bx)))
                    if got0 is not None:
                        assert (np.abs(got0 - want0) <= b0).all(), (order, known, alias, si)
                    results.setdefault((order, known), []).append((got, got0))
    for rs in results.values():                                              # every route of one case computes the same bits
        assert all(np.array_equal(r[0].view(np.uint32), rs[0][0].view(np.uint32)) for r in rs)
        x0s = [r[1] for r in rs if r[1] is not None]
        assert all(np.array_equal(v.view(np.uint32), x0s[0].view(np.uint32)) for v in x0s)


def test_nan_history_is_not_read_by_a_first_order_step(lib, data):
    for n, off in ((1024, 0), (1027, 1)):
        h = dict(data, x0_prev=np.full(1028, np.nan, np.float32))
        for src in sources(lib, FIRST):
            got, got0 = run(lib, FIRST, h, n, off, True, "x0", src)          # the NaN buffer is also where x0 goes
            assert np.isfinite(got).all() and np.isfinite(got0).all()
            x, eps = padded(data["x"][:n], off)[1], padded(data["eps"][:n], off)[1]
            kn = {k: padded(data[k][:n], off)[1] for k in ("orig", "orig_noise", "mask")}
            ref = _steps.dpm_step(lib, x, eps, padded(np.zeros(n, np.float32), off)[1], x0_prev=None, x0_out=None, **kn, **src)
            assert np.array_equal(bits(ref), got.view(np.uint32))


def test_vector_and_scalar_paths_give_the_same_bits(lib, data):
    for row in (FIRST, SECOND):
        for known in (False, True):
            src = sources(lib, row)[0]
            a, a0 = run(lib, row, data, 1024, 0, known, "none", src)         # every tensor 16-byte aligned, n % 4 == 0: vectors
            b, b0 = run(lib, row, data, 1024, 1, known, "none", src)         # the same values 4 bytes further on: element by element
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32)) and np.array_equal(a0.view(np.uint32), b0.view(np.uint32))


def test_order_1_is_the_ddim_step(lib, data):
    """One pf_dpm_step (c_1 = 0) and one pf_ddim_step (sigma = 0) on the same inputs, each against its own float64 evaluation with its own
    float32 coefficients; the two float64 values differ by the coefficients' rounding only."""
    n = 1024
    ts = dpm_ref.grid_logsnr(AB, 10)
    cur, tgt = AB[ts[9]], AB[ts[8]]
    dd = np.array([np.sqrt(1 - cur), np.sqrt(cur), np.sqrt(tgt), np.sqrt(1 - tgt), 0.0, np.sqrt(cur), np.sqrt(1 - cur)]).astype(np.float32)
    x, eps = data["x"][:n], data["eps"][:n]
    xd, ed = torch.from_numpy(x.copy()).cuda(), torch.from_numpy(eps.copy()).cuda()
    got_dpm = _steps.dpm_step(lib, xd, ed, torch.empty_like(xd), coef=_lib.DpmCoef(*(float(v) for v in FIRST))).cpu().numpy()
    got_ddim = _steps.ddim_step(lib, xd, ed, torch.empty_like(xd), coef=_lib.DdimCoef(*(float(v) for v in dd))).cpu().numpy()
    want_dpm = dpm_ref.update(FIRST, x, eps)[0]
    b_dpm = dpm_ref.budget(FIRST, x, eps)[0]
    # DDIM in float64 with ITS coefficients, and its budget by the same counting: mul, sub, div (pred_x0), mul, mul, add = 6 roundings on
    # |sqrt_aprev*pred_x0| + |dir_coef*eps|; the rounding of s1m*eps inside pred_x0 is covered while sqrt_aprev*s1m/sqrt_a <= 4*dir_coef
    s1m, sqrt_a, sqrt_ap, dirc = (float(v) for v in dd[:4])
    assert sqrt_ap * s1m / sqrt_a <= 4 * dirc
    p0 = (x.astype(np.float64) - s1m * eps.astype(np.float64)) / sqrt_a
    want_ddim = sqrt_ap * p0 + dirc * eps.astype(np.float64)
    b_ddim = 6 * dpm_ref.U * (np.abs(sqrt_ap * p0) + np.abs(dirc * eps.astype(np.float64)))
    assert (np.abs(got_dpm - want_dpm) <= b_dpm).all() and (np.abs(got_ddim - want_ddim) <= b_ddim).all()
    assert (np.abs(got_dpm.astype(np.float64) - got_ddim) <= b_dpm + b_ddim + np.abs(want_dpm - want_ddim)).all()
    print(f"dpm err/budget {np.max(np.abs(got_dpm - want_dpm) / b_dpm):.3f}, ddim err/budget {np.max(np.abs(got_ddim - want_ddim) / b_ddim):.3f}, "
          f"float64 values apart by {np.abs(want_dpm - want_ddim).max():.2e}")


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
def x_T():
    return torch.randn(2, 2, 8, 8, generator=torch.Generator().manual_seed(5))


@pytest.fixture(scope="module")
def gauss_runs(lib, x_T):
    """s -> {(family, steps): (float32 result, time step the loop starts at)}: every loop the tests below look at, run once."""
    cond = torch.zeros(2, 1, 4, device="cuda")
    out = {}
    for s in (0.5, 1.0, 4.0):
        m, r = GaussianDenoiser(s), {}
        for n in (10, 20, 40):
            sm = DPMSolverSampler(m, n)
            r[("2m", n)] = (sm.paint(x_T.cuda(), cond, len(sm.time_steps) - 1).cpu().numpy(), int(sm.time_steps[-1]), sm, m)
        sd = DDIMSampler(m, 50, "uniform", 0.0)
        r[("ddim", 50)] = (sd.paint(x_T.cuda(), cond, len(sd.time_steps) - 1).cpu().numpy(), int(sd.time_steps[-1]), sd, m)
        out[s] = r
    return out


@pytest.mark.parametrize("s", [0.5, 1.0, 4.0])
@pytest.mark.parametrize("n", [10, 20, 40])
def test_loop_stays_within_the_accumulated_budget_of_the_float64_loop(gauss_runs, x_T, s, n):
    got, _, sm, m = gauss_runs[s][("2m", n)]
    R = sm.coef_rows().astype(np.float64)
    want, bound = dpm_ref.loop_gauss_with_budget(R, m.gain32[sm.time_steps].astype(np.float64), x_T.numpy())
    err = np.abs(got - want)
    print(f"s={s} n={n}: max err {err.max():.3e}, max err/bound {np.max(err / bound):.3f}")
    assert (err <= bound).all(), float(np.max(err / bound))


@pytest.mark.parametrize("s", [0.5, 1.0, 4.0])
def test_float32_loops_reproduce_the_float64_solver_errors(gauss_runs, x_T, s):
    """Against the exact solution of the ODE: 2M at 10 logSNR steps beats DDIM at 50 uniform steps, and halving the step doubles the
    accuracy twice over (err(20) / err(40) >= 3).  These errors are 1e-3 and more, far above float32 rounding."""
    x = x_T.numpy()
    err = {k: dpm_ref.rel_err(v[0], dpm_ref.gauss_exact(AB, v[1], s, x)) for k, v in gauss_runs[s].items()}
    print(f"s={s}: " + ", ".join(f"{k[0]}@{k[1]} {e:.3e}" for k, e in err.items()))
    assert err[("2m", 10)] < err[("ddim", 50)]
    assert err[("2m", 20)] / err[("2m", 40)] >= 3
    print("float64: " + f"2m@10 {dpm_ref.err_2m(AB, 10, s):.3e}, ddim@50 {dpm_ref.err_ddim(AB, 50, s):.3e}")


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
    x, cond, orig, noise = (torch.randn(*s, generator=g).cuda() for s in ((2, 2, 16, 16), (2, 1, 32), (2, 2, 16, 16), (2, 2, 16, 16)))
    mask = (torch.rand(2, 2, 16, 16, generator=g) > 0.5).float().cuda()
    return x, cond, orig, noise, mask


@pytest.mark.parametrize("known", [False, True])
@pytest.mark.parametrize("scale", [1.0, 5.0])
def test_paint_eager_graph_repeat_and_fresh_history(ldm, known, scale):
    x, cond, orig, noise, mask = unet_inputs()
    kw = dict(uncond_scale=scale, uncond_cond=-torch.ones(2, 1, 32).cuda())
    if known:
        kw.update(orig=orig, mask=mask, orig_noise=noise)
    eager = DPMSolverSampler(ldm, 6)
    t = len(eager.time_steps) - 1
    assert t == 5
    a = eager.paint(x.clone(), cond, t, **kw)
    assert torch.isfinite(a).all()
    other = eager.paint(-x, cond, t, **kw)                                   # leaves ITS history behind ...
    assert not torch.equal(a, other)
    assert torch.equal(eager.paint(x.clone(), cond, t, **kw), a)             # ... which the next call does not see: same bits as the first
    assert torch.equal(DPMSolverSampler(ldm, 6).paint(x.clone(), cond, t, **kw), a)          # ... and as a fresh sampler's
    graph = DPMSolverSampler(ldm, 6, graph=True)
    b = graph.paint(x.clone(), cond, t, **kw)
    assert graph.graph_captures == 1 and torch.equal(a, b)
    assert torch.equal(graph.paint(-x, cond, t, **kw), other)
    assert torch.equal(graph.paint(x.clone(), cond, t, **kw), a) and graph.graph_captures == 1
    # a call that starts lower on the grid has another first-order row: own table, same captured step
    low = eager.paint(x.clone(), cond, 3, **kw)
    assert torch.equal(graph.paint(x.clone(), cond, 3, **kw), low) and graph.graph_captures == 1
    assert not torch.equal(low, a)
    if known:                                                                # the known region ends as the noised original of the last index
        row = eager.coef_rows()[0]
        keep = mask == 1
        assert torch.allclose(a[keep], (float(row[5]) * orig + float(row[6]) * noise)[keep], atol=1e-6)


def test_second_order_differs_from_first_and_order_1_tracks_ddim(ldm):
    x, cond, *_ = unet_inputs()
    two = DPMSolverSampler(ldm, 6, "uniform")
    one = DPMSolverSampler(ldm, 6, "uniform", order=1)
    dd = DDIMSampler(ldm, 6, "uniform", 0.0)
    assert np.array_equal(two.time_steps, dd.time_steps)
    t = len(dd.time_steps) - 1
    a, b, c = (s.paint(x.clone(), cond, t) for s in (two, one, dd))
    assert not torch.equal(a, b)
    assert (b - c).abs().max() < 1e-3 * c.abs().max()                        # the same first-order solver (the bar of the multi-step parity tests)
    assert (a - c).abs().max() > 10 * (b - c).abs().max()


def test_a_grid_that_repeats_time_steps_gives_a_finite_result(ldm):
    x, cond, *_ = unet_inputs()
    s = DPMSolverSampler(ldm, 50, "quad")
    assert len(set(s.time_steps.tolist())) < len(s.time_steps)
    out = s.paint(x.clone(), cond, len(s.time_steps) - 1)
    assert torch.isfinite(out).all()


def test_sample_q_sample_and_p_sample(ldm):
    x, cond, orig, noise, _ = unet_inputs()
    s = DPMSolverSampler(ldm, 6)
    t = len(s.time_steps) - 1
    assert torch.equal(s.sample(list(x.shape), cond, x_last=x.clone()), s.paint(x.clone(), cond, t))
    assert torch.equal(s.sample(list(x.shape), cond, x_last=x.clone(), t_start=2), s.paint(x.clone(), cond, t - 2))
    row = s.coef_rows()[3]
    assert torch.allclose(s.q_sample(orig, 3, noise), float(row[5]) * orig + float(row[6]) * noise, atol=1e-6)
    # two lone steps chained by hand are the first two steps of the loop
    seen = []
    s.on_step = lambda step, v: seen.append(v.clone())
    s.paint(x.clone(), cond, t)
    s.on_step = None
    prep = s.prepare(cond)
    x1, p0, _ = s.p_sample(x.clone(), cond, None, int(s.time_steps[t]), t, prep=prep)
    x2, _, _ = s.p_sample(x1, cond, None, int(s.time_steps[t - 1]), t - 1, prep=prep, x0_prev=p0)
    assert torch.equal(x1, seen[0]) and torch.equal(x2, seen[1])


# ---------------------------------------------------------------------------------------------- the CLI
def test_cli_writes_its_midi_file(tmp_path):
    import yaml
    params = dict(model_name="small_chd", in_channels=2, out_channels=2, channels=32, attention_levels=[1], n_res_blocks=1,
                  channel_multipliers=[1, 2], n_heads=2, tf_layers=1, d_cond=32, linear_start=0.00085, linear_end=0.012, n_steps=1000,
                  latent_scaling_factor=0.18215, img_h=128, img_w=128, cond_type="chord", cond_mode="mix", use_enc=True,
                  chd_n_step=32, chd_input_dim=36, chd_z_input_dim=32, chd_hidden_dim=64, chd_z_dim=32)
    (tmp_path / "params.yaml").write_text(yaml.safe_dump(params))
    out = tmp_path / "out"
    cmd = [sys.executable, "-m", "polyffusion_amd.inference_sdf", "--custom_params_path", str(tmp_path / "params.yaml"), "--synthetic_weights",
           "--synthetic", "--length", "1", "--dpm", "--dpm_steps", "4", "--seed", "9", "--output_dir", str(out)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300, env=dict(os.environ, PYTHONPATH=REPO), cwd=REPO)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    mids = [f for f in os.listdir(out) if f.endswith(".mid")]
    npys = [f for f in os.listdir(out) if f.endswith(".npy")]
    assert len(mids) == 1 and os.path.getsize(out / mids[0]) > 0 and len(npys) == 1
    assert np.isfinite(np.load(out / npys[0])).all()
