"""The stochastic DPM-Solver++(2M) on the GPU (-m gpu): ``pf_dpm_sde_step`` against the float64 restatement in ``tests/dpm_sde_ref.py``
on every route (first and second order, known region, the aliasings, coefficients by value and from a device table, noise from a tensor
and drawn in the kernel), what it must not touch or read, ``DPMSolverSampler(eta=1)`` on the closed-form Gaussian denoiser - rounding
against the float64 loop fed the same noise, the final variance against its closed form, sharding - and on a small synthetic UNet (eager
== captured graph, seeds, eta = 0 unchanged), steering with the history moved to the survivors, and the CLI.

Error budgets (``dpm_sde_ref.budget``): the roundings counted beside the kernel times 2^-24 times the sum of the term magnitudes."""
import glob
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import dpm_ref  # noqa: E402
import dpm_sde_ref as ref  # noqa: E402
from polyffusion_amd import _lib, _steps  # noqa: E402
from polyffusion_amd.arch import UNetConfig  # noqa: E402
from polyffusion_amd.sampler import DPMSolverSampler, Steering  # noqa: E402

AB = dpm_ref.alpha_bar()
TS = dpm_ref.grid_logsnr(AB, 20)
ROWS64 = ref.rows(AB, TS, eta=1.0)
ROWS = ROWS64.astype(np.float32)                  # the shipped schedule's 20-step rows at eta = 1, as the kernel gets them
FIRST, SECOND = ROWS[len(TS) - 1], ROWS[len(TS) // 2]
assert FIRST[4] == 0 and SECOND[4] != 0 and FIRST[7] != 0 and SECOND[7] != 0
assert (np.abs(ROWS64[:, 3]) / (4 * ROWS64[:, 1] * ROWS64[:, 2])).max() < 0.5      # budget()'s precondition, with margin
QUIET = ref.rows(AB, TS, eta=0.0).astype(np.float32)                               # the same grid with sigma_n == 0
PAD = 8                 # floats of sentinel on either side of an output (32 bytes: the payload keeps its 16-byte alignment)
SENTINEL = -777.25
NAMES = ("x", "eps", "x0_prev", "orig", "orig_noise", "mask", "noise")
SEED, DRAW, EOFF = 2024, 2 ** 32 + 5, 64          # a draw index above 2^32 and a nonzero element offset


@pytest.fixture(scope="module")
def lib():
    _lib.require_gpu()
    return _lib.load()


@pytest.fixture(scope="module")
def data(lib):
    """name -> float32 numpy array of 1028 elements (read-only); "drawn": what pf_randn(SEED, DRAW, EOFF) stores."""
    g = torch.Generator().manual_seed(11)
    d = {k: torch.randn(1028, generator=g).numpy() for k in NAMES if k != "mask"}
    m = (torch.rand(1028, generator=g) > 0.3).float()
    m[::7] = 0.25                                                            # a few soft mask values: the blend's products then round
    d["mask"] = m.numpy()
    d["drawn"] = _steps.randn(lib, (1028,), "cuda", SEED, DRAW, EOFF).cpu().numpy()
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


def sources(lib, row, others=ROWS):
    """The two coefficient sources: a host struct, and row 2 of a four-row device table with state = {index 2, draws DRAW}."""
    table = torch.from_numpy(np.stack([others[1], others[7], row, others[3]])).cuda()
    state = torch.zeros(2, dtype=torch.int64, device="cuda")
    _lib.check(lib.pf_step_state_set(state.data_ptr(), 2, DRAW, _lib.current_stream()), "pf_step_state_set")
    return dict(coef=_lib.DpmSdeCoef(*(float(v) for v in row))), dict(table=table, state=state)


def bits(a):
    return (a.cpu().numpy() if isinstance(a, torch.Tensor) else a).view(np.uint32)


def run(lib, row, h, n, off, known, alias, src, rng):
    """One launch on the leading n elements of the host data `h`; returns (x_out, x0 or None) as numpy after checking the sentinels.
    alias: "none" | "x" (x_out is x) | "x0" (x0_out is x0_prev) | "nox0" (x0_out NULL).  rng: draw in the kernel (the draw index by value -
    a state that is given overrides it with the same number) instead of reading h["noise"]."""
    dev = {k: padded(h[k][:n], off) for k in NAMES}
    out_w, out = dev["x"] if alias == "x" else padded(np.zeros(n, np.float32), off)
    if alias == "nox0":
        x0_w, x0 = None, None
    else:
        x0_w, x0 = dev["x0_prev"] if alias == "x0" else padded(np.zeros(n, np.float32), off)
    kw = dict(orig=dev["orig"][1], orig_noise=dev["orig_noise"][1], mask=dev["mask"][1]) if known else {}
    kw.update(dict(rng=(SEED, 0 if "state" in src else DRAW, EOFF)) if rng else dict(noise=dev["noise"][1]))
    _steps.dpm_sde_step(lib, dev["x"][1], dev["eps"][1], out, x0_prev=dev["x0_prev"][1], x0_out=x0, **kw, **src)
    torch.cuda.synchronize()
    assert untouched(out_w, n, off) and (x0_w is None or untouched(x0_w, n, off))
    for k in NAMES:                                                          # inputs are read-only, unless they are an aliased output
        if not (k == "x" and alias == "x") and not (k == "x0_prev" and alias == "x0"):
            assert np.array_equal(dev[k][1].cpu().numpy(), h[k][:n], equal_nan=True) and untouched(dev[k][0], n, off)
    return out.cpu().numpy(), None if x0 is None else x0.cpu().numpy()


def all_routes(lib, data, n, off, rng):
    """Every route of the four cases (order x known region) at one size: each within its budget of float64, all routes of a case the same
    bits.  rng: the noise is drawn in the kernel and must be what pf_randn stores.  Returns case -> (x_out, x0) of the first route."""
    h = dict(data, noise=data["drawn"]) if rng else data
    first = {}
    for order, row in (("first", FIRST), ("second", SECOND)):
        for known in (False, True):
            kn = {k: h[k][:n] for k in ("orig", "orig_noise", "mask")} if known else {}
            want, want0 = ref.update(row, h["x"][:n], h["eps"][:n], h["x0_prev"][:n], h["noise"][:n], **kn)
            bx, b0 = ref.budget(row, h["x"][:n], h["eps"][:n], h["x0_prev"][:n], h["noise"][:n], **kn)
            rs = []
            for alias in ("none", "x", "x0", "nox0"):
                for si, src in enumerate(sources(lib, row)):
                    got, got0 = run(lib, row, h, n, off, known, alias, src, rng)
                    ex = np.abs(got - want)
                    print(f"n={n} rng={rng} {order} known={known} alias={alias} src={si}: max err/budget {np.max(ex / bx):.3f}")
                    assert (ex <= bx).all(), (order, known, alias, si, float(np.max(ex / bx)))
                    if got0 is not None:
                        assert (np.abs(got0 - want0) <= b0).all(), (order, known, alias, si)
                    rs.append((got, got0))
            assert all(np.array_equal(bits(r[0]), bits(rs[0][0])) for r in rs)
            x0s = [r[1] for r in rs if r[1] is not None]
            assert all(np.array_equal(bits(v), bits(x0s[0])) for v in x0s)
            first[(order, known)] = rs[0]
    return first


# ---------------------------------------------------------------------------------------------- one update
@pytest.mark.parametrize("n", [1, 4, 7, 1027])
def test_one_update_with_tensor_noise_is_within_its_rounding_budget_of_float64(lib, data, n):
    all_routes(lib, data, n, 1 if n == 1027 else 0, rng=False)               # the last size from a base 4 bytes past a 16-byte boundary


@pytest.mark.parametrize("n", [4, 8, 1024, 1028])
def test_in_kernel_noise_equals_randn_plus_the_tensor_form_bit_for_bit(lib, data, n):
    drawn = all_routes(lib, data, n, 0, rng=True)
    h = dict(data, noise=data["drawn"])
    for (order, known), (got, got0) in drawn.items():
        row = FIRST if order == "first" else SECOND
        want, want0 = run(lib, row, h, n, 0, known, "none", sources(lib, row)[0], rng=False)
        assert np.array_equal(bits(got), bits(want)) and np.array_equal(bits(got0), bits(want0))


def test_vector_and_scalar_paths_give_the_same_bits(lib, data):
    for row in (FIRST, SECOND):
        for known in (False, True):
            src = sources(lib, row)[0]
            a, a0 = run(lib, row, data, 1024, 0, known, "none", src, False)  # every tensor 16-byte aligned, n % 4 == 0: vectors
            b, b0 = run(lib, row, data, 1024, 1, known, "none", src, False)  # the same values 4 bytes further on: element by element
            assert np.array_equal(bits(a), bits(b)) and np.array_equal(bits(a0), bits(b0))


# ---------------------------------------------------------------------------------------------- sigma_n == 0
def test_a_row_without_noise_has_the_bits_of_pf_dpm_step_and_reads_neither_noise_nor_a_first_order_history(lib, data):
    nan = np.full(1028, np.nan, np.float32)
    for n, off in ((1024, 0), (1027, 1)):
        for row in (QUIET[len(TS) - 1], QUIET[len(TS) // 2]):
            assert row[7] == 0
            second = row[4] != 0
            h = dict(data, noise=nan) if second else dict(data, noise=nan, x0_prev=nan)
            for known in (False, True):
                dev = {k: padded(data[k][:n], off)[1] for k in NAMES}
                kw = dict(orig=dev["orig"], orig_noise=dev["orig_noise"], mask=dev["mask"]) if known else {}
                x0 = torch.empty_like(dev["x"])
                want = _steps.dpm_step(lib, dev["x"], dev["eps"], torch.empty_like(dev["x"]), coef=_lib.DpmCoef(*(float(v) for v in row[:7])),
                                       x0_prev=dev["x0_prev"] if second else None, x0_out=x0, **kw)
                for src in sources(lib, row, QUIET):
                    got, got0 = run(lib, row, h, n, off, known, "none", src, False)
                    assert np.isfinite(got).all() and np.array_equal(bits(got), bits(want)) and np.array_equal(bits(got0), bits(x0))
                    if off == 0:                                             # the in-kernel form makes no Philox call either: the same bits
                        got, _ = run(lib, row, h, n, off, known, "none", src, True)
                        assert np.array_equal(bits(got), bits(want))


# ---------------------------------------------------------------------------------------------- refusals
def test_argument_refusals_return_the_message_and_launch_nothing(lib, data):
    n = 16
    t = lambda: padded(data["x"][:n])
    (xw, x), (ew, e), (ow, out), (nw, nz) = t(), t(), t(), t()
    noisy, second = _lib.DpmSdeCoef(*(float(v) for v in FIRST)), _lib.DpmSdeCoef(*(float(v) for v in SECOND))
    for pattern, kw in (("needs a noise tensor or rng", dict(coef=noisy)),
                        ("needs x0_prev", dict(coef=second, noise=nz)),
                        ("noise tensor must be NULL", dict(coef=noisy, noise=nz, rng=(SEED, 0, 0))),
                        ("multiples of 4", dict(coef=noisy, rng=(SEED, 0, 2))),
                        ("all three or none", dict(coef=noisy, noise=nz, orig=x)),
                        ("both by value", dict(coef=noisy, noise=nz, table=x, state=torch.zeros(2, dtype=torch.int64, device="cuda")))):
        with pytest.raises(RuntimeError, match=pattern):
            _steps.dpm_sde_step(lib, x, e, out, **kw)
    with pytest.raises(RuntimeError, match="16-byte aligned"):
        _steps.dpm_sde_step(lib, xw[PAD + 1: PAD + 1 + n], e, out, coef=noisy, rng=(SEED, 0, 0))
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), data["x"][:n]) and untouched(ow, n)


# ---------------------------------------------------------------------------------------------- the loop on the analytic denoiser
class GaussianDenoiser:
    """Stands in for a LatentDiffusion: the optimal denoiser of data ~ N(0, s^2), eps = gain[t] * x as ONE float32 product on the device.
    Carries what the samplers touch: n_steps, alpha_bar, an eps_model with the two prepare hooks, and the table steering predicts x0 with."""

    def __init__(self, s):
        self.n_steps = 1000
        self.alpha_bar = torch.from_numpy(AB.astype(np.float32))
        self.eps_model = self
        self.gain32 = dpm_ref.gauss_gain(AB, np.arange(1000), s).astype(np.float32)
        self.gain = torch.from_numpy(self.gain32).cuda()
        self._x0t = _steps.x0_threshold_table(self.alpha_bar).cuda()

    def prepare_time(self, n, out=None):
        return None

    def prepare_cond(self, ctx, out=None):
        return None

    def x0_threshold_table(self, device):
        return self._x0t

    def __call__(self, x, t, c, time_table=None, cross_bias=None):
        return x * self.gain[t].view(-1, 1, 1, 1)


def drawn_noises(lib, shape, seed, n, first=0, offset=0):
    """Draws first .. first + n - 1 of the sampler's generator for a tensor of `shape`, read back with pf_randn."""
    return [_steps.randn(lib, shape, "cuda", seed, first + k, offset).cpu().numpy() for k in range(n)]


@pytest.fixture(scope="module")
def gauss(lib):
    m = GaussianDenoiser(1.0)
    x_T = torch.randn(4, 2, 16, 128, generator=torch.Generator().manual_seed(5))
    s = DPMSolverSampler(m, 20, eta=1.0, seed=7)
    assert np.array_equal(s.time_steps, TS)
    got = s.paint(x_T.cuda(), torch.zeros(4, 1, 4, device="cuda"), len(TS) - 1).cpu().numpy()
    assert s._draws == len(TS)                                               # one draw index per step
    return m, x_T, s, got, drawn_noises(lib, x_T.shape, 7, len(TS))


def test_loop_stays_within_the_accumulated_budget_of_the_float64_loop_fed_the_same_noise(gauss):
    m, x_T, s, got, noises = gauss
    R = s.sde_coef_rows().astype(np.float64)
    want, bound = ref.loop_gauss_with_budget(R, m.gain32[TS].astype(np.float64), x_T.numpy(), noises)
    err = np.abs(got - want)
    print(f"max err {err.max():.3e}, max err/bound {np.max(err / bound):.3f}")
    assert (err <= bound).all(), float(np.max(err / bound))


def test_final_variance_is_the_closed_form_prediction(gauss):
    """x_T ~ N(0, 1), so the prediction starts from variance 1; n independent Gaussian values estimate a variance to sqrt(2/n) of it."""
    m, x_T, s, got, _ = gauss
    pred = ref.gauss_cov(s.sde_coef_rows().astype(np.float64), m.gain32[TS].astype(np.float64), 1.0)
    var, n = float(np.mean(got.astype(np.float64) ** 2)), got.size
    print(f"sample variance {var:.5f}, predicted {pred:.5f}, off by {abs(var / pred - 1):.4f} of it (allowed {5 * np.sqrt(2 / n):.4f})")
    assert abs(var / pred - 1) <= 5 * np.sqrt(2 / n)


def test_a_shard_draws_the_rows_of_the_whole_run(gauss):
    m, x_T, _, got, _ = gauss
    part = DPMSolverSampler(m, 20, eta=1.0, seed=7, sample_offset=2).paint(x_T[2:4].cuda(), torch.zeros(2, 1, 4, device="cuda"), len(TS) - 1)
    assert np.array_equal(bits(part), bits(got[2:4]))


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
@pytest.mark.parametrize("scale", [1.0, 3.0])
def test_paint_eager_equals_graph_and_seeds_and_draw_state(ldm, known, scale):
    x, cond, orig, noise, mask = unet_inputs()
    kw = dict(uncond_scale=scale, uncond_cond=-torch.ones(2, 1, 32).cuda())
    if known:
        kw.update(orig=orig, mask=mask, orig_noise=noise)
    make = lambda **k: DPMSolverSampler(ldm, 6, eta=1.0, **{**dict(seed=4), **k})
    eager = make()
    t = len(eager.time_steps) - 1
    a = eager.paint(x.clone(), cond, t, **kw)
    assert torch.isfinite(a).all() and eager._draws == t + 1
    assert torch.equal(make().paint(x.clone(), cond, t, **kw), a)            # one seed: identical
    assert not torch.equal(make(seed=5).paint(x.clone(), cond, t, **kw), a)  # another seed differs
    graph = make(graph=True)
    b = graph.paint(x.clone(), cond, t, **kw)
    assert graph.graph_captures == 1 and torch.equal(a, b) and graph._draws == t + 1
    # a second call goes on with the draw counter and with nothing else: a fresh sampler put at that counter gives the same bits
    other = eager.paint(-x, cond, t, **kw)
    fresh = make()
    fresh._draws = t + 1
    assert torch.equal(fresh.paint(-x, cond, t, **kw), other) and not torch.equal(other, -a)
    assert torch.equal(graph.paint(-x, cond, t, **kw), other) and graph.graph_captures == 1
    # eta = 0 is the sampler as it was: pf_dpm_step, the same bits, no draw
    plain, zero = DPMSolverSampler(ldm, 6, seed=4), DPMSolverSampler(ldm, 6, eta=0.0, seed=4)
    p = plain.paint(x.clone(), cond, t, **kw)
    assert torch.equal(zero.paint(x.clone(), cond, t, **kw), p) and zero._draws == 0 and not torch.equal(p, a)
    assert torch.equal(DPMSolverSampler(ldm, 6, eta=0.0, seed=4, graph=True).paint(x.clone(), cond, t, **kw), p)


def test_p_sample_honours_temperature_and_repeat_noise(ldm):
    x, cond, *_ = unet_inputs()
    s = DPMSolverSampler(ldm, 6, eta=1.0, seed=4)
    t = len(s.time_steps) - 1
    seen = []
    s.on_step = lambda step, v: seen.append(v.clone())
    s.paint(x.clone(), cond, t)
    s.on_step = None
    s._draws = 0
    x1, p0, _ = s.p_sample(x.clone(), cond, None, int(s.time_steps[t]), t)
    x2, _, _ = s.p_sample(x1, cond, None, int(s.time_steps[t - 1]), t - 1, x0_prev=p0)
    assert torch.equal(x1, seen[0]) and torch.equal(x2, seen[1])             # two lone steps are the first two of the loop
    s._draws = 0
    cold, _, _ = s.p_sample(x.clone(), cond, None, int(s.time_steps[t]), t, temperature=0.0)
    s._draws = 0
    rep, _, _ = s.p_sample(x[:1].expand(2, -1, -1, -1).contiguous(), cond[:1].expand(2, -1, -1).contiguous(), None, int(s.time_steps[t]), t, repeat_noise=True)
    assert not torch.equal(cold, x1) and torch.equal(rep[0], rep[1])


# ---------------------------------------------------------------------------------------------- steering
def test_steering_moves_the_history_with_the_survivors(lib):
    m = GaussianDenoiser(1.0)
    x_T = torch.randn(8, 2, 8, 16, generator=torch.Generator().manual_seed(6))
    cond = torch.zeros(8, 1, 4, device="cuda")

    def favour_one(x0):                                                      # particle 1 of each group of 4
        r = torch.zeros(8, dtype=torch.float64, device=x0.device)
        r[1::4] = 1.0
        return r

    st = Steering(n=4, reward=favour_one, lam=50.0, every=2, ess=1.0)
    s = DPMSolverSampler(m, 20, eta=1.0, seed=9, steering=st)
    got = s.paint(x_T.cuda(), cond, len(TS) - 1).cpu().numpy()
    rec = s.last_steering
    assert rec.steps == list(range(1, len(TS) - 1, 2)) and not np.array_equal(rec.lineage(), np.tile(np.arange(4), (2, 1)))
    ancestors = {k: (np.arange(8) // 4) * 4 + a.cpu().numpy() for k, a in zip(rec.steps, rec.ancestors)}
    assert all((a % 4 == 1).all() for a in ancestors.values())
    R = s.sde_coef_rows().astype(np.float64)
    noises = drawn_noises(lib, x_T.shape, 9, len(TS))
    want, bound = ref.loop_gauss_with_budget(R, m.gain32[TS].astype(np.float64), x_T.numpy(), noises, ancestors)
    err = np.abs(got - want)
    print(f"steered: max err/bound {np.max(err / bound):.3f}")
    assert (err <= bound).all(), float(np.max(err / bound))
    # had the history stayed behind, the result would be far outside the bound
    stale, _ = ref.loop_gauss_with_budget(R, m.gain32[TS].astype(np.float64), x_T.numpy(), noises, ancestors, history_moves=False)
    assert not (np.abs(got - stale) <= bound).all()
    # lam = 0: the weights are uniform, every particle is its own ancestor - the unsteered run, bit for bit
    flat = DPMSolverSampler(m, 20, eta=1.0, seed=9, steering=Steering(n=4, reward=favour_one, lam=0.0, every=2, ess=1.0))
    plain = DPMSolverSampler(m, 20, eta=1.0, seed=9)
    assert torch.equal(flat.paint(x_T.cuda(), cond, len(TS) - 1), plain.paint(x_T.cuda(), cond, len(TS) - 1))


# ---------------------------------------------------------------------------------------------- the CLI
def test_cli_steers_the_stochastic_loop_and_records_it(tmp_path):
    from polyffusion_amd import inference_sdf
    out = tmp_path / "s"
    argv = ["--params_preset", "sdf_chd8bar", "--synthetic_weights", "--synthetic", "--length", "1", "--seed", "5", "--precision", "bf16x3",
            "--dpm", "--dpm_steps", "6", "--dpm_eta", "1", "--num_generate", "1", "--best_of", "2", "--steer", "--steer_every", "2",
            "--output_dir", str(out)]
    assert inference_sdf.main(argv) == 0
    mids = glob.glob(os.path.join(str(out), "*.mid"))
    assert len(mids) == 1 and os.path.getsize(mids[0]) > 0 and "dpm_eta=1" in mids[0] and "steer=" in mids[0]
    doc = json.load(open(glob.glob(os.path.join(str(out), "*_score.json"))[0]))
    sd = doc["steer"]
    assert (sd["sampler"], sd["eta"], sd["every"], sd["n"]) == ("dpm", 1.0, 2, 2) and len(sd["ranks"][0]["events"]["steps"]) >= 1
