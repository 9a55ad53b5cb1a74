"""Joint overlapping-window sampling on the GPU (-m gpu): ``pf_window_split`` against slicing and ``pf_window_merge`` against the float32
and float64 restatements in ``tests/window_ref.py``, on both of their paths and inside sentinel guards; the merge's folded guidance combine
against ``pf_cfg_combine`` / ``pf_cfg_combine3`` followed by a plain merge; ``DiffusionSampler.windows`` through the three sampler families
on the small UNet of ``tests/test_gpu_guidance.py`` and on an elementwise denoiser; and the CLI's ``--joint``.

Every comparison is bit for bit except the one against float64, whose budget per canvas element is
``(2k + 2) * 2^-24 * (sum_j w_j |e_j| / sum_j w_j) * (1 + 2^-10)`` for a row under k windows (k products and k - 1 sums on either side of the
division, and the division; ``window_ref.budget``), and exactly zero where k = 1."""
import functools
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import window_ref  # noqa: E402
from polyffusion_amd import _lib, _steps  # noqa: E402
from polyffusion_amd.arch import UNetConfig  # noqa: E402
from polyffusion_amd.sampler import DDIMSampler, DPMSolverSampler, DualScale, SDFSampler, WindowPlan  # noqa: E402
from polyffusion_amd.unet import LatentDiffusion, UNetModel  # noqa: E402
from polyffusion_amd.weights import synth_unet_state  # noqa: E402

PAD = 8                 # floats of sentinel on either side of a buffer (32 bytes: the payload keeps its alignment)
SENTINEL = -777.25
SPLIT = 12              # chord part of the 32-wide condition of the small UNet

#        S  C  Hw  W  Wn stride
CASES = [(2, 2, 8, 4, 3, 4),        # plain half overlap
         (1, 3, 8, 5, 4, 3),        # odd W: scalar path, k = 3
         (2, 2, 8, 4, 2, 8),        # no overlap
         (1, 2, 16, 4, 5, 4),       # k = 4
         (1, 2, 8, 4, 7, 1),        # k = 8, the cap
         (1, 1, 12, 3, 4, 5)]
SCALES = (1e-3, 1.0, 30.0)          # magnitudes of the windows' values, one per batch row in turn


@pytest.fixture(scope="module")
def lib():
    _lib.require_gpu()
    return _lib.load()


def bits(a):
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else a
    return np.ascontiguousarray(a).view(np.uint32)


def padded(values, off):
    """(whole buffer, payload view shaped like `values`) on the device: the payload starts `off` floats past a 16-byte boundary."""
    values = np.asarray(values, dtype=np.float32)
    n = values.size
    whole = torch.full((n + 2 * PAD + 4,), SENTINEL, device="cuda")
    assert whole.data_ptr() % 16 == 0
    view = whole[PAD + off: PAD + off + n]
    view.copy_(torch.from_numpy(values.reshape(-1).copy()))
    assert view.data_ptr() % 16 == 4 * off
    return whole, view.view(values.shape)


def untouched(whole, n, off):
    w = whole.cpu().numpy()
    return (w[: PAD + off] == SENTINEL).all() and (w[PAD + off + n:] == SENTINEL).all()


@functools.lru_cache(maxsize=None)
def reference(case, blend):
    """Inputs and expected results of one case, computed once and never written to again."""
    S, C, Hw, W, Wn, stride = case
    rng = np.random.default_rng(1000 * CASES.index(case) + window_ref.BLENDS.index(blend))
    hc = window_ref.canvas_h(Wn, stride, Hw)
    canvas = rng.standard_normal((S, C, hc, W)).astype(np.float32)
    eps = rng.standard_normal((S * Wn, C, Hw, W)).astype(np.float32)
    eps *= np.array([SCALES[i % 3] for i in range(S * Wn)], dtype=np.float32).reshape(-1, 1, 1, 1)
    w = window_ref.weights(Hw, stride, blend)
    bound, k = window_ref.budget(eps, w, S, Wn, stride)
    ref = dict(canvas=canvas, windows=window_ref.split(canvas, Wn, stride, Hw), eps=eps, w=w, m32=window_ref.merge32(eps, w, S, Wn, stride),
               m64=window_ref.merge64(eps, w, S, Wn, stride), bound=bound, k=k)
    for v in ref.values():
        v.setflags(write=False)
    return ref


def merge(lib, eps, w, out, case, groups=1, scales=()):
    S, C, Hw, W, Wn, stride = case
    got = _steps.window_merge(lib, eps, w, S, Wn, stride, groups, scales, out=out)
    torch.cuda.synchronize()
    return got


# ---------------------------------------------------------------------------------------------- the two kernels
@pytest.mark.parametrize("off", [0, 1])
@pytest.mark.parametrize("blend", window_ref.BLENDS)
@pytest.mark.parametrize("case", CASES, ids=lambda c: "x".join(map(str, c)))
def test_split_is_slicing_bit_for_bit(lib, case, blend, off):
    S, C, Hw, W, Wn, stride = case
    ref = reference(case, blend)
    cw, cv = padded(ref["canvas"], off)
    ow, ov = padded(np.zeros_like(ref["windows"]), off)
    before = cw.clone()
    _lib.check(lib.pf_window_split(cv.data_ptr(), ov.data_ptr(), S, C, Hw, W, Wn, stride, _lib.current_stream()), "pf_window_split")
    torch.cuda.synchronize()
    sliced = torch.stack([cv[s, :, j * stride: j * stride + Hw, :] for s in range(S) for j in range(Wn)])
    assert torch.equal(ov, sliced) and np.array_equal(bits(ov), bits(ref["windows"]))
    assert untouched(ow, ov.numel(), off) and torch.equal(cw, before)
    # the library's own wrapper allocates: the same bits
    assert torch.equal(_steps.window_split(lib, cv.contiguous(), Wn, stride, Hw), sliced)


@pytest.mark.parametrize("off", [0, 1])
@pytest.mark.parametrize("blend", window_ref.BLENDS)
@pytest.mark.parametrize("case", CASES, ids=lambda c: "x".join(map(str, c)))
def test_merge_is_its_float32_restatement_and_within_the_float64_budget(lib, case, blend, off):
    ref = reference(case, blend)
    ew, ev = padded(ref["eps"], off)
    ww, wv = padded(ref["w"], off)
    ow, ov = padded(np.zeros_like(ref["m32"]), off)
    e_before, w_before = ew.clone(), ww.clone()
    got = merge(lib, ev, wv, ov, case).cpu().numpy()
    assert np.array_equal(bits(got), bits(ref["m32"]))
    assert untouched(ow, ov.numel(), off) and torch.equal(ew, e_before) and torch.equal(ww, w_before)
    err = np.abs(got.astype(np.float64) - ref["m64"])
    used = float(np.max(err[ref["bound"] > 0] / ref["bound"][ref["bound"] > 0])) if (ref["bound"] > 0).any() else 0.0
    print(f"{case} {blend} off {off}: k up to {ref['k'].max()}, max err {err.max():.3e}, largest share of the budget {used:.3f}")
    assert (err <= ref["bound"]).all(), used
    one = ref["k"] == 1
    assert (err[:, :, one, :] == 0).all() and (ref["bound"][:, :, one, :] == 0).all()
    S, C, Hw, W, Wn, stride = case
    assert ref["k"].max() == min(Wn, -(-Hw // stride))


@pytest.mark.parametrize("blend", window_ref.BLENDS)
@pytest.mark.parametrize("case", CASES, ids=lambda c: "x".join(map(str, c)))
def test_merge_with_groups_is_the_combine_then_the_plain_merge(lib, case, blend):
    S, C, Hw, W, Wn, stride = case
    n = S * Wn * C * Hw * W
    g = torch.Generator().manual_seed(5 + CASES.index(case))
    e3 = torch.randn(3 * S * Wn, C, Hw, W, generator=g).cuda()
    w = torch.from_numpy(window_ref.weights(Hw, stride, blend)).cuda()
    out = lambda: torch.empty(S, C, window_ref.canvas_h(Wn, stride, Hw), W, device="cuda")
    comb = torch.empty(S * Wn, C, Hw, W, device="cuda")
    e2 = e3[: 2 * S * Wn].contiguous()
    _lib.check(lib.pf_cfg_combine(e2.data_ptr(), 2.5, comb.data_ptr(), n, _lib.current_stream()), "pf_cfg_combine")
    want = merge(lib, comb, w, out(), case)
    assert torch.equal(merge(lib, e2, w, out(), case, 2, (2.5,)), want)
    _lib.check(lib.pf_cfg_combine3(e3.data_ptr(), 3.0, 1.5, comb.data_ptr(), n, _lib.current_stream()), "pf_cfg_combine3")
    want3 = merge(lib, comb, w, out(), case)
    assert torch.equal(merge(lib, e3, w, out(), case, 3, (3.0, 1.5)), want3) and not torch.equal(want3, want)
    assert torch.isfinite(want3).all()


@pytest.mark.parametrize("blend", window_ref.BLENDS)
@pytest.mark.parametrize("shape", [(2, 2, 8, 4), (1, 3, 8, 5)])
def test_one_window_is_the_identity(lib, shape, blend):
    S, C, Hw, W = shape
    e = torch.randn(S, C, Hw, W, generator=torch.Generator().manual_seed(3)).cuda()
    w = torch.from_numpy(window_ref.weights(Hw, Hw // 2, blend)).cuda()      # any positive weights: a lone window is a select
    case = (S, C, Hw, W, 1, Hw // 2)
    assert torch.equal(merge(lib, e, w, torch.empty_like(e), case), e)
    assert torch.equal(_steps.window_split(lib, e, 1, Hw // 2, Hw), e)


# ---------------------------------------------------------------------------------------------- the samplers
def small(levels=(1,), d_cond=32):
    kw = dict(in_channels=2, out_channels=2, channels=32, n_res_blocks=1, attention_levels=levels, channel_multipliers=(1, 2),
              n_heads=1 if 0 in levels else 2, tf_layers=1, d_cond=d_cond)          # d_head must be 32 or 64
    m = UNetModel(img_h=32, img_w=32, **kw)
    m.load_state_dict(synth_unet_state(UNetConfig(**kw), 0))
    return m


@pytest.fixture(scope="module")
def net():
    _lib.require_gpu()
    return small()


class Elementwise:
    """eps = G * x + P * cond[column I]: every element on its own, one rounded torch operation at a time - so a sample's eps does not depend
    on which batch it is evaluated in, which no tiled UNet promises bit for bit."""
    G, P, I = 0.75, 0.5, 2

    def prepare_time(self, n, out=None):
        return None

    def prepare_cond(self, ctx, out=None):
        return None

    def __call__(self, x, t, c, time_table=None, cross_bias=None, shared_x=False):
        if shared_x:
            x = torch.cat([x] * (2 if shared_x is True else int(shared_x)))
        return x * self.G + c[:, 0, self.I].view(-1, 1, 1, 1) * self.P


FAMILIES = {
    "ddpm": lambda ldm, **kw: SDFSampler(ldm, seed=3, **kw),
    "ddim": lambda ldm, **kw: DDIMSampler(ldm, 20, "uniform", 0.0, seed=3, **kw),
    "ddim_eta1": lambda ldm, **kw: DDIMSampler(ldm, 20, "uniform", 1.0, seed=3, **kw),     # every step draws its noise in the update kernel
    "dpm": lambda ldm, **kw: DPMSolverSampler(ldm, 6, seed=3, **kw),
}
OVERLAP = dict(S=2, Wn=3, stride=16)            # canvases of 64 rows under three half-overlapping windows of the 32-row UNet


def canvas_inputs(S, Wn, stride, seed=9):
    g = torch.Generator().manual_seed(seed)
    hc = stride * (Wn - 1) + 32
    x = torch.randn(S, 2, hc, 32, generator=g).cuda()
    c = torch.randn(S * Wn, 1, 32, generator=g).cuda()
    known = dict(orig=torch.rand(S, 2, hc, 32, generator=g).cuda(), mask=(torch.rand(S, 2, hc, 32, generator=g) > 0.5).float().cuda(),
                 orig_noise=torch.randn(S, 2, hc, 32, generator=g).cuda())
    return x, c, -torch.ones_like(c), known


def to_batch(v, Wn):
    """A canvas under windows that do not overlap, as the batch of its windows: [S, C, Wn * 32, W] -> [S * Wn, C, 32, W]."""
    S, C, _, W = v.shape
    return v.reshape(S, C, Wn, 32, W).permute(0, 2, 1, 3, 4).reshape(S * Wn, C, 32, W).contiguous()


@pytest.mark.parametrize("blend", window_ref.BLENDS)
@pytest.mark.parametrize("scale", [1.0, 2.5, DualScale(3.0, 1.5, SPLIT)], ids=["scale1", "scale2.5", "dual"])
def test_get_eps_is_split_flat_get_eps_and_the_reference_merge(net, scale, blend):
    S, Wn, stride = OVERLAP["S"], OVERLAP["Wn"], OVERLAP["stride"]
    x, c, uc, _ = canvas_inputs(S, Wn, stride)
    ldm = LatentDiffusion(net)
    plan = WindowPlan(Wn, stride, 32, blend)
    t = torch.full((S * Wn,), 500, device="cuda")
    windows = torch.stack([x[s, :, j * stride: j * stride + 32, :] for s in range(S) for j in range(Wn)]).contiguous()
    flat = SDFSampler(ldm, seed=3).get_eps(windows, t, c, uncond_scale=scale, uncond_cond=uc).cpu().numpy()
    want = window_ref.merge32(flat, plan.weights(), S, Wn, stride)
    s = SDFSampler(ldm, seed=3, windows=plan)
    got = s.get_eps(x, t, c, uncond_scale=scale, uncond_cond=uc)
    assert got.shape == x.shape and np.array_equal(bits(got), bits(want))
    prep = s.prepare(c, uncond_scale=scale, uncond_cond=uc)
    assert torch.equal(s.get_eps(x, t, c, uncond_scale=scale, uncond_cond=uc, prep=prep), got)
    with pytest.raises(ValueError):
        s.get_eps(x[:, :, :48], t, c, uncond_scale=scale, uncond_cond=uc)           # not this plan's canvas
    with pytest.raises(ValueError):
        s.get_eps(x, t[:S], c, uncond_scale=scale, uncond_cond=uc)                  # one time step per window


@pytest.mark.parametrize("known", [False, True], ids=["free", "known"])
@pytest.mark.parametrize("graph", [False, True], ids=["eager", "captured"])
@pytest.mark.parametrize("family", ["ddpm", "ddim_eta1", "dpm"])
def test_a_plan_of_one_window_is_the_plain_sampler(net, family, graph, known):
    x, c, uc, kn = canvas_inputs(2, 1, 16)
    kn = kn if known else {}
    outs = []
    for plan in (None, WindowPlan(1, 16, 32, "ramp")):
        s = FAMILIES[family](LatentDiffusion(net), graph=graph, windows=plan)
        outs.append(s.paint(x, c, 3, uncond_scale=2.5, uncond_cond=uc, **kn))
        assert s.graph_captures == int(graph)
    assert torch.equal(outs[0], outs[1]) and torch.isfinite(outs[0]).all()
    if family == "ddpm" and not graph and not known:
        a, b = (FAMILIES[family](LatentDiffusion(net), windows=p) for p in (None, WindowPlan(1, 32, 32)))
        assert torch.equal(a.sample(list(x.shape), c, x_last=x, t_start=997), b.sample(list(x.shape), c, x_last=x, t_start=997))
        assert torch.equal(a.p_sample(x, c, None, 500, uncond_scale=2.5, uncond_cond=uc)[0], b.p_sample(x, c, None, 500, uncond_scale=2.5, uncond_cond=uc)[0])


@pytest.mark.parametrize("family", ["ddim", "dpm"])
def test_windows_that_do_not_overlap_are_the_plain_sampler_on_the_rearranged_batch(net, family):
    S, Wn = 2, 2
    x, c, uc, kn = canvas_inputs(S, Wn, 32)
    s = FAMILIES[family](LatentDiffusion(net), windows=WindowPlan(Wn, 32, 32))
    got = s.paint(x, c, 3, uncond_scale=2.5, uncond_cond=uc, **kn)
    plain = FAMILIES[family](LatentDiffusion(net))
    want = plain.paint(to_batch(x, Wn), c, 3, uncond_scale=2.5, uncond_cond=uc, **{k: to_batch(v, Wn) for k, v in kn.items()})
    assert got.shape == x.shape and torch.equal(to_batch(got, Wn), want)
    assert torch.equal(s.sample(list(x.shape), c, x_last=x, t_start=len(s.time_steps) - 3), to_batch_inverse(plain.sample(None, c, x_last=to_batch(x, Wn), t_start=len(s.time_steps) - 3), S, Wn))


def to_batch_inverse(v, S, Wn):
    _, C, _, W = v.shape
    return v.reshape(S, Wn, C, 32, W).permute(0, 2, 1, 3, 4).reshape(S, C, Wn * 32, W).contiguous()


@pytest.mark.parametrize("family", ["ddpm", "ddim", "ddim_eta1", "dpm"])
def test_the_captured_loop_is_the_eager_loop_and_the_coupling_enters(net, family):
    S, Wn, stride = OVERLAP["S"], OVERLAP["Wn"], OVERLAP["stride"]
    x, c, uc, kn = canvas_inputs(S, Wn, stride)
    plan = WindowPlan(Wn, stride, 32, "ramp")
    run = lambda smp, **kw: smp.paint(x, c, 3, uncond_scale=2.5, uncond_cond=uc, **kw)
    e = FAMILIES[family](LatentDiffusion(net), windows=plan)
    eager, again = run(e, **kn), run(e, **kn)                                      # (a second call goes on in the noise stream)
    assert eager.shape == x.shape and torch.isfinite(eager).all()
    g = FAMILIES[family](LatentDiffusion(net), graph=True, windows=plan)
    assert torch.equal(run(g, **kn), eager) and g.graph_captures == 1
    assert torch.equal(run(g, **kn), again) and g.graph_captures == 1            # the same shapes: the same captured step
    g.windows = e.windows = WindowPlan(Wn, stride, 32, "mean")                    # another plan with the same shapes captures again
    other = run(g, **kn)
    assert g.graph_captures == 2 and not torch.equal(other, eager) and not torch.equal(other, again)
    assert torch.equal(other, run(e, **kn))
    # the windows on their own (no canvas): where two of them overlap, the joint run is neither - the blend entered
    free = run(FAMILIES[family](LatentDiffusion(net), windows=plan))
    alone = FAMILIES[family](LatentDiffusion(net))
    windows = torch.stack([x[s, :, j * stride: j * stride + 32, :] for s in range(S) for j in range(Wn)]).contiguous()
    indep = alone.paint(windows, c, 3, uncond_scale=2.5, uncond_cond=uc)
    assert not torch.equal(free[0, :, :32], indep[0]) and not torch.equal(free[0, :, 16:48], indep[1])


@pytest.mark.parametrize("family", ["ddpm", "ddim_eta1"])
def test_a_shard_that_holds_song_1_draws_and_computes_what_the_whole_run_does_for_it(family):
    """On the elementwise denoiser, where a song's eps does not depend on its batch: noise is keyed by the global song index."""
    S, Wn, stride = OVERLAP["S"], OVERLAP["Wn"], OVERLAP["stride"]
    x, c, uc, kn = canvas_inputs(S, Wn, stride, seed=11)
    plan = WindowPlan(Wn, stride, 32, "ramp")
    whole = FAMILIES[family](LatentDiffusion(Elementwise()), windows=plan).paint(x, c, 3, uncond_scale=2.5, uncond_cond=uc, **kn)
    shard = FAMILIES[family](LatentDiffusion(Elementwise()), windows=plan, sample_offset=1)
    one = shard.paint(x[1:].contiguous(), c[Wn:].contiguous(), 3, uncond_scale=2.5, uncond_cond=uc[Wn:].contiguous(),
                      **{k: v[1:].contiguous() for k, v in kn.items()})
    assert torch.equal(one[0], whole[1]) and torch.isfinite(whole).all()
    unkeyed = FAMILIES[family](LatentDiffusion(Elementwise()), windows=plan).paint(
        x[1:].contiguous(), c[Wn:].contiguous(), 3, uncond_scale=2.5, uncond_cond=uc[Wn:].contiguous(), **{k: v[1:].contiguous() for k, v in kn.items()})
    assert not torch.equal(unkeyed[0], whole[1])                                  # the offset is what makes them agree


# ---------------------------------------------------------------------------------------------- the CLI
def cli(out, *flags):
    from polyffusion_amd import inference_sdf
    argv = ["--params_preset", "sdf_chd8bar", "--synthetic_weights", "--synthetic", "--dpm", "--dpm_steps", "3", "--seed", "7",
            "--output_dir", str(out)] + list(flags)
    assert inference_sdf.main(argv) == 0
    mids = [f for f in os.listdir(out) if f.endswith(".mid")]
    npys = [f for f in os.listdir(out) if f.endswith(".npy")]
    assert len(mids) == 1 and len(npys) == 1 and os.path.getsize(out / mids[0]) > 0
    return mids[0], np.load(out / npys[0])


def test_cli_joint_writes_a_song_of_two_segments_and_repeats_under_a_seed(tmp_path):
    runs = []
    for name in ("a", "b"):
        mid, roll = cli(tmp_path / name, "--length", "2", "--joint")
        assert ",joint]" in mid and mid.startswith("sdf_chd8bar")
        runs.append(roll)
    assert runs[0].shape == (2, 2, 128, 128) and np.isfinite(runs[0]).all()
    assert np.array_equal(bits(runs[0]), bits(runs[1]))


def test_cli_joint_on_one_segment_is_the_plain_run(tmp_path):
    mid_j, joint = cli(tmp_path / "joint", "--length", "1", "--joint")
    mid_p, plain = cli(tmp_path / "plain", "--length", "1")
    assert "joint" in mid_j and "joint" not in mid_p
    assert joint.shape == plain.shape == (1, 2, 128, 128) and np.array_equal(bits(joint), bits(plain))
