"""Dual classifier-free guidance on the GPU (-m gpu): ``pf_cfg_combine3`` bit for bit against its formula on both of its paths, the
shared-prefix plan over three groups (``UNetModel.forward(shared_x=3)``, ``pf_unet_forward_cfgn``) against the concatenated batch and the
CPU oracle, ``DualScale`` through the three sampler families - its two reductions bit-identical to the float path, eager == captured step -
one guided evaluation on an analytic denoiser against the float64 restatement in ``tests/guidance_ref.py``, and the CLI.

Bounds: shared against concatenated batch and against the oracle are ``tests/test_gpu_cfg_share.py``'s for the same comparison (the same
kernels, the same cause of difference: the smaller prefix batch may pick other tiles).  ``share_cfg_prefix`` on / off keeps that file's 1e-4
at scales (3, 5): the combine weights |1 - 3| + |3 - 5| + |5| = 9 sum to what guidance 5 gives there (|1 - 5| + |5|)."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import guidance_ref  # noqa: E402
from oracle import unet_ref  # noqa: E402
from polyffusion_amd import _lib  # noqa: E402
from polyffusion_amd.arch import UNetConfig  # noqa: E402
from polyffusion_amd.sampler import DDIMSampler, DPMSolverSampler, DualScale, SDFSampler, guidance_plan  # noqa: E402
from polyffusion_amd.unet import LatentDiffusion, UNetModel  # noqa: E402
from polyffusion_amd.weights import synth_unet_state  # noqa: E402

PAD = 8                 # floats of sentinel on either side of a buffer (32 bytes: the payload keeps its alignment)
SENTINEL = -777.25
SPLIT = 12              # chord part of the 32-wide condition of the small UNet


@pytest.fixture(scope="module")
def lib():
    _lib.require_gpu()
    return _lib.load()


def bits(t):
    return t.detach().cpu().numpy().view(np.uint32)


# ---------------------------------------------------------------------------------------------- pf_cfg_combine3
def padded(values, off):
    """(whole buffer, payload view) on the device: the payload starts `off` floats past a 16-byte boundary, sentinels around it."""
    n = len(values)
    whole = torch.full((n + 2 * PAD + 4,), SENTINEL, device="cuda")
    assert whole.data_ptr() % 16 == 0
    view = whole[PAD + off: PAD + off + n]
    view.copy_(torch.from_numpy(np.asarray(values, dtype=np.float32)))
    return whole, view


def untouched(whole, n, off):
    w = whole.cpu().numpy()
    return (w[: PAD + off] == SENTINEL).all() and (w[PAD + off + n:] == SENTINEL).all()


@pytest.fixture(scope="module")
def eps3():
    e = torch.randn(3, 4096, generator=torch.Generator().manual_seed(21)).numpy()
    e.setflags(write=False)
    return e


@pytest.mark.parametrize("n", [1, 3, 4, 5, 1027, 4096])
def test_combine3_is_its_formula_bit_for_bit_on_both_paths(lib, eps3, n):
    s1, s2 = 3.0, 1.5
    stacked = np.concatenate([eps3[0, :n], eps3[1, :n], eps3[2, :n]])
    want = guidance_ref.combine3_f32(eps3[0, :n], eps3[1, :n], eps3[2, :n], s1, s2)
    for in_off in (0, 1):
        for out_off in (0, 1):
            src_w, src = padded(stacked, in_off)
            dst_w, dst = padded(np.zeros(n, np.float32), out_off)
            _lib.check(lib.pf_cfg_combine3(src.data_ptr(), s1, s2, dst.data_ptr(), n, _lib.current_stream()), "pf_cfg_combine3")
            torch.cuda.synchronize()
            assert np.array_equal(bits(dst), want.view(np.uint32)), (n, in_off, out_off)
            assert untouched(dst_w, n, out_off) and untouched(src_w, 3 * n, in_off)
            assert np.array_equal(src.cpu().numpy(), stacked)                    # the input is read only
    # e1 == e2: the second term is s2 * 0 - the two-way combine's bits on [e0 | e1]
    two = np.concatenate([eps3[0, :n], eps3[1, :n]])
    for off in (0, 1):
        _, src3 = padded(np.concatenate([two, eps3[1, :n]]), off)
        _, src2 = padded(two, off)
        _, a = padded(np.zeros(n, np.float32), off)
        _, b = padded(np.zeros(n, np.float32), off)
        _lib.check(lib.pf_cfg_combine3(src3.data_ptr(), s1, s2, a.data_ptr(), n, _lib.current_stream()), "pf_cfg_combine3")
        _lib.check(lib.pf_cfg_combine(src2.data_ptr(), s1, b.data_ptr(), n, _lib.current_stream()), "pf_cfg_combine")
        assert np.array_equal(bits(a), bits(b)) and np.array_equal(bits(b), guidance_ref.combine2_f32(eps3[0, :n], eps3[1, :n], s1).view(np.uint32))


def test_combine3_refuses_null_pointers_and_an_empty_tensor(lib):
    buf = torch.full((16,), SENTINEL, device="cuda")
    for args in ((None, 1.0, 2.0, buf.data_ptr(), 4), (buf.data_ptr(), 1.0, 2.0, None, 4), (buf.data_ptr(), 1.0, 2.0, buf.data_ptr(), 0)):
        assert lib.pf_cfg_combine3(*args, _lib.current_stream()) < 0
        assert "cfg_combine3: bad arguments" in lib.pf_last_error().decode()
    torch.cuda.synchronize()
    assert (buf == SENTINEL).all()


# ---------------------------------------------------------------------------------------------- the plan over three groups
def small(levels=(1,), d_cond=32):
    kw = dict(in_channels=2, out_channels=2, channels=32, n_res_blocks=1, attention_levels=levels, channel_multipliers=(1, 2),
              n_heads=1 if 0 in levels else 2, tf_layers=1, d_cond=d_cond)          # d_head must be 32 or 64
    m = UNetModel(img_h=32, img_w=32, **kw)
    cfg = UNetConfig(**kw)
    m.load_state_dict(synth_unet_state(cfg, 0))
    return m, cfg


def raw_forward(lib, m, entry, x, t, cond, rows, groups):
    """`entry` (pf_unet_forward_cfg, or pf_unet_forward_cfgn with `groups`) called directly on a workspace of the group plan's size."""
    ws = m.workspace(rows, cond.shape[1], groups)
    out = torch.empty(rows, m.cfg.out_channels, m.img_h, m.img_w, device="cuda")
    head = (m._h, x.data_ptr(), t.data_ptr(), cond.data_ptr(), rows)
    tail = (cond.shape[1], None, out.data_ptr(), ws.data_ptr(), ws.numel(), _lib.current_stream())
    rc = lib.pf_unet_forward_cfgn(*head, groups, *tail) if entry == "cfgn" else lib.pf_unet_forward_cfg(*head, *tail)
    _lib.check(rc, entry)
    return out


@pytest.mark.parametrize("precision", ["f32", "bf16x3"])
@pytest.mark.parametrize("levels", [(1,), (0, 1), ()])
def test_three_groups_share_the_prefix(lib, levels, precision):
    m, cfg = small(levels)
    m.set_precision(precision)
    g = torch.Generator().manual_seed(5)
    B = 3
    x, c = torch.randn(B, 2, 32, 32, generator=g).cuda(), torch.randn(B, 1, 32, generator=g).cuda()
    uc = -torch.ones_like(c)
    t = torch.tensor([7, 999, 400]).cuda()
    t3, c3 = torch.cat([t, t, t]), torch.cat([uc, DualScale(3, 5, SPLIT).partial(c, uc), c])
    ref = m(torch.cat([x, x, x]), t3, c3).clone()
    got = m(x, t3, c3, shared_x=3).clone()
    d = (got - ref).abs().max().item()
    print(f"three groups, shared prefix [{levels}, {precision}] vs concatenated batch: {d:.2e}")
    assert d <= (2e-5 if precision == "f32" else 1e-4)
    assert not torch.equal(got[:B], got[B: 2 * B]) and not torch.equal(got[B: 2 * B], got[2 * B:]) and not torch.equal(got[:B], got[2 * B:])
    w = unet_ref.to_torch(synth_unet_state(cfg, 0))
    with torch.no_grad():
        o = unet_ref.unet_forward(w, cfg, torch.cat([x, x, x]).cpu(), t3.cpu(), c3.cpu())
    err = (got.cpu() - o).abs().max().item()
    print(f"  vs oracle: {err:.2e}")
    assert err < (1e-4 if precision == "f32" else 5e-4)
    assert torch.equal(m(x, t3, c3, shared_x=3), got)                            # bit-reproducible
    table, cross = m.prepare_time(1001), m.prepare_cond(c3)
    assert torch.equal(m(x, t3, c3, shared_x=3, time_table=table, cross_bias=cross, check_t=True), got)
    same = m(x, t3, torch.cat([c, c, c]), shared_x=3)                            # equal conditions -> bit-equal groups
    assert torch.equal(same[:B], same[B: 2 * B]) and torch.equal(same[:B], same[2 * B:])
    assert m.n_launches(3 * B, shared_x=3) == m.n_launches(3 * B) + 6
    # two groups through the new entry: the existing entry's bits
    t2, c2 = torch.cat([t, t]), torch.cat([uc, c])
    old = raw_forward(lib, m, "cfg", x, t2, c2, 2 * B, 2)
    assert torch.equal(raw_forward(lib, m, "cfgn", x, t2, c2, 2 * B, 2), old) and torch.equal(m(x, t2, c2, shared_x=True), old)
    assert torch.equal(m(x, t2, c2, shared_x=2), old)
    # refusals: groups that carry different t (under check_t), row counts that are no multiple of three
    bad_t = torch.cat([t, t, t.flip(0)])
    with pytest.raises(RuntimeError, match="groups of time_steps"):
        m(x, bad_t, c3, shared_x=3, check_t=True)
    with pytest.raises(RuntimeError):
        m(x, t3[:-1], c3[:-1], shared_x=3)
    with pytest.raises(RuntimeError):
        m(x, torch.cat([t, t]), torch.cat([uc, c]), shared_x=3)
    ws = m.workspace(3 * B, 1, 3)
    assert lib.pf_unet_forward_cfgn(m._h, x.data_ptr(), t3.data_ptr(), c3.data_ptr(), 3 * B - 1, 3, 1, None, got.data_ptr(), ws.data_ptr(), ws.numel(),
                                    _lib.current_stream()) < 0


# ---------------------------------------------------------------------------------------------- the samplers
@pytest.fixture(scope="module")
def net():
    _lib.require_gpu()
    return small()[0]


def inputs():
    g = torch.Generator().manual_seed(9)
    x, c = torch.randn(2, 2, 32, 32, generator=g).cuda(), torch.randn(2, 1, 32, generator=g).cuda()
    return x, c, -torch.ones_like(c)


FAMILIES = {
    "ddpm": lambda ldm, **kw: SDFSampler(ldm, seed=3, **kw),
    "ddim": lambda ldm, **kw: DDIMSampler(ldm, 20, "uniform", 0.0, seed=3, **kw),
    "dpm": lambda ldm, **kw: DPMSolverSampler(ldm, 6, seed=3, **kw),
}


def run(family, net, scale, cond, uc, graph=False, share=True, lone_step=False):
    """A 4-step loop of `family` (or, for DDPM with `lone_step`, one p_sample) from the same x."""
    x = inputs()[0]
    s = FAMILIES[family](LatentDiffusion(net), graph=graph)
    s.share_cfg_prefix = share
    if lone_step:
        return s.p_sample(x, cond, None, 500, uncond_scale=scale, uncond_cond=uc)[0]
    return s.paint(x, cond, 3, uncond_scale=scale, uncond_cond=uc)


@pytest.mark.parametrize("family", list(FAMILIES))
def test_reductions_are_the_float_path_and_the_captured_step_is_the_eager_loop(net, family):
    _, c, uc = inputs()
    lone = family == "ddpm"                                                      # DDPM: the reductions on p_sample, the graph on paint
    for order in guidance_ref.ORDERS:
        part = DualScale(2, 1, SPLIT, order).partial(c, uc)
        for s in (2.5, 1.0):
            assert torch.equal(run(family, net, DualScale(s, s, SPLIT, order), c, uc, lone_step=lone), run(family, net, s, c, uc, lone_step=lone))
            assert torch.equal(run(family, net, DualScale(s, 0.0, SPLIT, order), c, uc, lone_step=lone), run(family, net, s, part, uc, lone_step=lone))
    ds = DualScale(3.0, 1.5, SPLIT)
    eager = run(family, net, ds, c, uc)
    assert torch.isfinite(eager).all()
    assert torch.equal(run(family, net, ds, c, uc, graph=True), eager)
    # only the second scale, or only the order, changes the result; so does the single scale
    assert not torch.equal(run(family, net, DualScale(3.0, 2.5, SPLIT), c, uc), eager)
    assert not torch.equal(run(family, net, DualScale(3.0, 1.5, SPLIT, "txt,chd"), c, uc), eager)
    assert not torch.equal(run(family, net, 3.0, c, uc), eager)


def test_one_captured_step_serves_equal_dual_scales(net):
    x, c, uc = inputs()
    s = DDIMSampler(LatentDiffusion(net), 20, "uniform", 0.0, seed=3, graph=True)
    a = s.paint(x, c, 3, uncond_scale=DualScale(3.0, 1.5, SPLIT), uncond_cond=uc)
    b = s.paint(x, c, 3, uncond_scale=DualScale(3, 1.5, SPLIT, "chd,txt"), uncond_cond=uc)
    assert s.graph_captures == 1 and torch.equal(a, b)
    s.paint(x, c, 3, uncond_scale=DualScale(3.0, 1.5, SPLIT, "txt,chd"), uncond_cond=uc)
    assert s.graph_captures == 2


def test_get_eps_is_the_combine_of_the_three_group_forward(lib, net):
    x, c, uc = inputs()
    ldm = LatentDiffusion(net)
    s = SDFSampler(ldm, seed=3)
    t = torch.tensor([500, 500]).cuda()
    for order in guidance_ref.ORDERS:
        ds = DualScale(3.0, 5.0, SPLIT, order)
        ctx, groups, scales = guidance_plan(c, ds, uc)
        assert groups == 3 and scales == (3.0, 5.0)
        e3 = ldm(x, torch.cat([t, t, t]), ctx, shared_x=3).clone()
        want = torch.empty_like(e3[:2])
        _lib.check(lib.pf_cfg_combine3(e3.data_ptr(), 3.0, 5.0, want.data_ptr(), want.numel(), _lib.current_stream()), "pf_cfg_combine3")
        assert torch.equal(s.get_eps(x, t, c, uncond_scale=ds, uncond_cond=uc), want)
        assert torch.equal(s.get_eps(x, t, c, uncond_scale=ds, uncond_cond=uc, prep=s.prepare(c, uncond_scale=ds, uncond_cond=uc)), want)


@pytest.mark.parametrize("graph", [False, True])
def test_with_and_without_the_shared_prefix(net, graph):
    x, c, uc = inputs()
    ds = DualScale(3.0, 5.0, SPLIT)
    outs = []
    for share in (True, False):
        d = DDIMSampler(LatentDiffusion(net), 20, "uniform", 0.0, seed=5, graph=graph)
        d.share_cfg_prefix = share
        outs.append(d.paint(x, c, 5, uncond_scale=ds, uncond_cond=uc))
    d = (outs[0] - outs[1]).abs().max().item()
    print(f"share_cfg_prefix on vs off, scales (3, 5), 6 DDIM steps, graph={graph}: {d:.2e}")
    assert d < 1e-4 and torch.isfinite(outs[0]).all()


class LinearDenoiser:
    """eps = G * x + P * cond[chord column] + Q * cond[texture column]: linear in x and in the condition, three products and two sums, each
    one rounded torch operation.  No ``supports_shared_x``: ``get_eps`` repeats x per group."""
    n_steps = 1000
    G, P, Q, I, J = 0.75, 0.5, -1.25, 2, 20                                    # I < SPLIT <= J

    def __init__(self):
        self.eps_model = self
        self.rows = None

    def prepare_time(self, n, out=None):
        return None

    def prepare_cond(self, ctx, out=None):
        return None

    def __call__(self, x, t, c, time_table=None, cross_bias=None):
        self.rows = (x.shape[0], t.shape[0], c.shape[0])
        return (x * self.G + c[:, 0, self.I].view(-1, 1, 1, 1) * self.P) + c[:, 0, self.J].view(-1, 1, 1, 1) * self.Q

    @classmethod
    def f64(cls, x, c):
        return x * cls.G + c[:, 0, cls.I].reshape(-1, 1, 1, 1) * cls.P + c[:, 0, cls.J].reshape(-1, 1, 1, 1) * cls.Q

    @classmethod
    def budget(cls, x, c):
        """Five roundings of at most half an ulp, every intermediate bounded by the sum of the term magnitudes."""
        return 5 * 2.0 ** -24 * (np.abs(x * cls.G) + np.abs(c[:, 0, cls.I] * cls.P).reshape(-1, 1, 1, 1) + np.abs(c[:, 0, cls.J] * cls.Q).reshape(-1, 1, 1, 1))


@pytest.mark.parametrize("order", guidance_ref.ORDERS)
def test_guided_eps_on_an_analytic_denoiser_against_float64(order):
    """Budget, per element: each of the three evaluations carries its own five roundings into the result with the weight the telescoped
    formula gives it (|1 - s1|, |s1 - s2|, |s2|), and the combine adds five roundings of intermediates bounded by
    |e0| + |s1| |e1 - e0| + |s2| |e2 - e1|.  A factor 1 + 2^-10 covers the second-order terms."""
    s1, s2 = 3.0, 5.0
    m = LinearDenoiser()
    g = torch.Generator().manual_seed(13)
    x, c = torch.randn(2, 2, 8, 8, generator=g), torch.randn(2, 1, 32, generator=g)
    uc = -torch.ones(2, 1, 32)
    s = SDFSampler.__new__(SDFSampler)
    s.model, s.share_cfg_prefix, s._lib = m, True, _lib.load()
    got = s.get_eps(x.cuda(), torch.tensor([5, 5]).cuda(), c.cuda(), uncond_scale=DualScale(s1, s2, SPLIT, order), uncond_cond=uc.cuda()).cpu().numpy()
    assert m.rows == (6, 6, 6)
    x64, c64, u64 = x.double().numpy(), c.double().numpy(), uc.double().numpy()
    want = guidance_ref.dual(LinearDenoiser.f64, x64, c64, u64, s1, s2, SPLIT, order)
    part = guidance_ref.partial(c64, u64, SPLIT, order)
    e0, e1, e2 = (LinearDenoiser.f64(x64, v) for v in (u64, part, c64))
    b0, b1, b2 = (LinearDenoiser.budget(x64, v) for v in (u64, part, c64))
    bound = (abs(1 - s1) * b0 + abs(s1 - s2) * b1 + abs(s2) * b2
             + 5 * 2.0 ** -24 * (np.abs(e0) + abs(s1) * np.abs(e1 - e0) + abs(s2) * np.abs(e2 - e1))) * (1 + 2.0 ** -10)
    err = np.abs(got - want)
    print(f"order {order}: max err {err.max():.3e}, max err/bound {np.max(err / bound):.3f}")
    assert (err <= bound).all(), float(np.max(err / bound))
    # the partial condition did enter: the result differs from single-scale guidance with either scale
    assert np.abs(want - guidance_ref.single(LinearDenoiser.f64, x64, c64, u64, s1)).max() > 1e-2
    assert np.abs(want - guidance_ref.single(LinearDenoiser.f64, x64, c64, u64, s2)).max() > 1e-2


# ---------------------------------------------------------------------------------------------- the CLI
def test_cli_writes_a_stamp_that_names_both_scales_and_repeats_under_a_seed(tmp_path):
    from polyffusion_amd import inference_sdf
    runs = []
    for name in ("a", "b"):
        out = tmp_path / name
        argv = ["--params_preset", "sdf_chd8bar_txt", "--synthetic_weights", "--synthetic", "--length", "1", "--dpm", "--dpm_steps", "3",
                "--uncond_scale_chd", "3", "--uncond_scale_txt", "1.5", "--seed", "7", "--output_dir", str(out)]
        assert inference_sdf.main(argv) == 0
        mids = [f for f in os.listdir(out) if f.endswith(".mid")]
        npys = [f for f in os.listdir(out) if f.endswith(".npy")]
        assert len(mids) == 1 and len(npys) == 1 and os.path.getsize(out / mids[0]) > 0
        assert "[scale=chd:3.0,txt:1.5]" in mids[0] and mids[0].startswith("sdf_chd8bar_txt")
        runs.append(np.load(out / npys[0]))
    assert np.isfinite(runs[0]).all() and runs[0].shape == (1, 2, 128, 128)
    assert np.array_equal(runs[0].view(np.uint32), runs[1].view(np.uint32))
