"""Dual classifier-free guidance without a GPU (-m "not gpu"): the new C entry points are declared, exported and bound; the CLI flags and
their refusals; the ONE branch function ``prepare`` and ``get_eps`` share (``sampler.guidance_plan``) - group count, row order, combine
arguments and the partial condition for both orders against ``tests/guidance_ref.py``; ``DualScale`` as a key; the shared-prefix plan over
three groups counted on the host; and, in float64, the facts the reductions rest on."""
import os
import re

import numpy as np
import pytest
import torch

import guidance_ref
from polyffusion_amd import _lib
from polyffusion_amd.params import preset

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = 0x1000          # a non-null, 16-byte aligned address that a refused call never touches
EINVAL = -1          # PF_EINVAL (include/pfhip.h)
NEW = ("pf_cfg_combine3", "pf_unet_forward_cfgn", "pf_unet_workspace_bytes_cfgn", "pf_unet_n_launches_cfgn")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        from polyffusion_amd.build import build
        build(verbose=False)
    return _lib.load()


def test_header_declares_and_the_library_exports_the_new_entry_points(lib):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "pfhip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(pf_[a-z0-9_]+)\s*\(", hdr))
    for name in NEW:
        assert name in declared, f"{name} not declared in pfhip.h"
        assert name in _lib.SIGNATURES, f"{name} has no prototype in _lib.SIGNATURES"
        assert hasattr(lib, name), f"{name} not exported"


def test_combine3_refuses_bad_arguments_before_any_launch(lib):
    for args in ((None, 1.0, 2.0, FAKE, 8), (FAKE, 1.0, 2.0, None, 8), (FAKE, 1.0, 2.0, FAKE, 0)):
        assert lib.pf_cfg_combine3(*args, None) == EINVAL
        assert "cfg_combine3: bad arguments" in lib.pf_last_error().decode()


# ---- CLI ----------------------------------------------------------------------------------------------------------------
def _args(*argv):
    from polyffusion_amd.inference_sdf import make_parser
    return make_parser().parse_args(list(argv))


def test_parser_defaults_and_refusals():
    from polyffusion_amd.inference_sdf import dual_scale, wants_dual_guidance
    from polyffusion_amd.sampler import DualScale
    a = _args()
    assert a.uncond_scale_chd is None and a.uncond_scale_txt is None and a.guidance_order == "chd,txt" and a.uncond_scale == 1.0
    assert wants_dual_guidance(a, "chord+txt") is False and wants_dual_guidance(a, "chord") is False
    with pytest.raises(SystemExit):
        _args("--guidance_order", "chd")                                        # argparse: not one of the two orders
    for only in ("--uncond_scale_chd", "--uncond_scale_txt"):                    # both scales go together
        with pytest.raises(SystemExit, match="give both"):
            wants_dual_guidance(_args(only, "2"), "chord+txt")
    both = ("--uncond_scale_chd", "3", "--uncond_scale_txt", "1.5")
    for cond_type in ("chord", "txt", "pnotree"):                                # a one-part condition has nothing to steer separately
        with pytest.raises(SystemExit, match="chord\\+txt"):
            wants_dual_guidance(_args(*both), cond_type)
    with pytest.raises(SystemExit, match="not both"):                            # the single scale and the two exclude each other
        wants_dual_guidance(_args(*both, "--uncond_scale", "2"), "chord+txt")
    assert wants_dual_guidance(_args(*both, "--uncond_scale", "1.0"), "chord+txt") is True     # ... the default value is no single scale
    a = _args(*both)
    assert wants_dual_guidance(a, "chord+txt") is True
    assert dual_scale(a, 512) == DualScale(3.0, 1.5, 512, "chd,txt")
    b = _args(*both, "--guidance_order", "txt,chd")                              # X stays the chord's scale: it is now the SECOND term's
    assert dual_scale(b, 512) == DualScale(1.5, 3.0, 512, "txt,chd")
    assert dual_scale(a, 512).chd == dual_scale(b, 512).chd == 3.0 and dual_scale(a, 512).txt == dual_scale(b, 512).txt == 1.5
    from polyffusion_amd.inference_sdf import make_parser
    text = make_parser().format_help()
    assert "eps(chd,txt)" in re.sub(r"\s+", "", text) and "--guidance_order" in text


def test_stamp_names_both_scales():
    from polyffusion_amd.inference_sdf import Experiments
    from polyffusion_amd.sampler import DualScale

    class S:
        time_steps = [0]
    e = Experiments("sdf_chd8bar_txt", preset("sdf_chd8bar_txt"), S(), t_idx=0)
    assert "[scale=chd:3.0,txt:1.5]" in e._stamp(DualScale(3, 1.5, 512), False)
    assert "[scale=chd:3.0,txt:1.5,txt-first,autoreg]" in e._stamp(DualScale(1.5, 3, 512, "txt,chd"), True)
    assert "[scale=2.0]" in e._stamp(2.0, False)                                 # a float's stamp is what it was


# ---- the branch function -------------------------------------------------------------------------------------------------
B, D, K = 2, 8, 3


def _conds():
    g = torch.Generator().manual_seed(3)
    return torch.randn(B, 1, D, generator=g), -torch.ones(B, 1, D)


def test_guidance_plan_for_a_float_is_the_reference_branching():
    from polyffusion_amd.sampler import guidance_plan
    c, uc = _conds()
    for scale, want in ((1.0, c), (0.0, uc)):
        ctx, groups, args = guidance_plan(c, scale, uc)
        assert groups == 1 and args == () and ctx is want
    ctx, groups, args = guidance_plan(c, 2.5, None)
    assert groups == 1 and args == () and ctx is c
    ctx, groups, args = guidance_plan(c, 2.5, uc)
    assert groups == 2 and args == (2.5,) and torch.equal(ctx, torch.cat([uc, c]))


@pytest.mark.parametrize("order", guidance_ref.ORDERS)
def test_guidance_plan_for_a_dual_scale(order):
    from polyffusion_amd.sampler import DualScale, guidance_plan
    c, uc = _conds()
    part = torch.from_numpy(guidance_ref.partial(c.numpy(), uc.numpy(), K, order)).float()
    assert torch.equal(DualScale(2, 3, K, order).partial(c, uc), part)
    assert not torch.equal(part, c) and not torch.equal(part, uc.expand_as(c))
    keep = slice(0, K) if order == "chd,txt" else slice(K, D)
    assert torch.equal(part[..., keep], c[..., keep])                            # the part named first is the one kept
    # general case: three groups in the order [unconditional | partial | full], scales as given
    ctx, groups, args = guidance_plan(c, DualScale(3.0, 5.0, K, order), uc)
    assert guidance_ref.reduce(3.0, 5.0) == ("dual",)
    assert groups == 3 and args == (3.0, 5.0) and torch.equal(ctx, torch.cat([uc, part, c]))
    # first == second: exactly what the float gives, shortcuts included
    for s in (2.5, 1.0, 0.0):
        assert guidance_ref.reduce(s, s) == ("single", s, "cond")
        got, want = guidance_plan(c, DualScale(s, s, K, order), uc), guidance_plan(c, s, uc)
        assert got[1:] == want[1:] and torch.equal(got[0], want[0])
    # second == 0: the float path towards the partial condition
    for s in (2.5, 1.0):
        assert guidance_ref.reduce(s, 0.0) == ("single", s, "partial")
        got, want = guidance_plan(c, DualScale(s, 0.0, K, order), uc), guidance_plan(part, s, uc)
        assert got[1:] == want[1:] and torch.equal(got[0], want[0])
    # a one-row unconditional condition serves every sample (the autoregressive loop's uc)
    assert torch.equal(DualScale(2, 3, K, order).partial(c, uc[:1]), part)


def test_dual_scale_refusals():
    from polyffusion_amd.sampler import DualScale, guidance_plan
    c, uc = _conds()
    for split in (0, D, D + 1, -1):
        for first, second in ((3.0, 5.0), (2.0, 2.0), (2.0, 0.0)):            # also where a reduction would not need the split
            with pytest.raises(ValueError, match="split"):
                guidance_plan(c, DualScale(first, second, split), uc)
    with pytest.raises(ValueError, match="uncond_cond"):
        guidance_plan(c, DualScale(3.0, 5.0, K), None)
    with pytest.raises(ValueError, match="order"):
        DualScale(3.0, 5.0, K, "chd")


def test_dual_scale_is_a_value_and_keys_one_graph():
    from polyffusion_amd.sampler import DualScale, scale_key
    a, b = DualScale(3, 1.5, 512), DualScale(3.0, 1.5, 512, "chd,txt")
    assert a == b and hash(a) == hash(b) and len({a, b}) == 1
    assert scale_key(a) is a and {("ddim", scale_key(a)): 1}.get(("ddim", scale_key(b))) == 1
    assert len({a, DualScale(3, 1.5, 512, "txt,chd"), DualScale(3, 2.0, 512), DualScale(3, 1.5, 256)}) == 4
    assert scale_key(2) == 2.0 and isinstance(scale_key(2), float)
    with pytest.raises(Exception):
        a.first = 1.0                                                            # frozen


def test_prepare_and_get_eps_take_the_same_context():
    """Both go through guidance_plan: the context ``prepare`` collapses is the one ``get_eps`` hands to the model (stub model, CPU tensors)."""
    from polyffusion_amd.sampler import DiffusionSampler, DualScale, guidance_plan
    seen = {}

    class Eps:
        def prepare_time(self, n, out=None):
            return None

        def prepare_cond(self, ctx, out=None):
            seen["prepare"] = ctx
            return None

    class Model:
        n_steps, eps_model = 10, Eps()

        def __call__(self, x, t, ctx, **kw):
            seen["model"], seen["rows"] = ctx, (x.shape[0], t.shape[0])
            raise StopIteration                                                  # stop before the combine kernel (no GPU here)

    s = DiffusionSampler.__new__(DiffusionSampler)
    s.model, s.share_cfg_prefix = Model(), True
    c, uc = _conds()
    for scale in (2.5, DualScale(3.0, 5.0, K), DualScale(3.0, 5.0, K, "txt,chd"), DualScale(2.0, 0.0, K)):
        s.prepare(c, uncond_scale=scale, uncond_cond=uc)
        with pytest.raises(StopIteration):
            s.get_eps(torch.zeros(B, 1), torch.zeros(B, dtype=torch.long), c, uncond_scale=scale, uncond_cond=uc)
        ctx, groups, _ = guidance_plan(c, scale, uc)
        assert torch.equal(seen["prepare"], ctx) and torch.equal(seen["model"], ctx)
        assert seen["rows"] == (B * groups, B * groups)                          # no supports_shared_x: x is repeated per group


# ---- plan accounting ------------------------------------------------------------------------------------------------------
def _small(levels):
    from polyffusion_amd.unet import UNetModel
    return UNetModel(in_channels=2, out_channels=2, channels=32, n_res_blocks=1, attention_levels=levels, channel_multipliers=(1, 2),
                     n_heads=1 if 0 in levels else 2, tf_layers=1, d_cond=32, img_h=32, img_w=32)


def _full():
    from polyffusion_amd.inference_sdf import build_unet
    return build_unet(preset("sdf_chd8bar_txt"))


@pytest.mark.parametrize("make,Bs", [(lambda: _small((1,)), (1, 3)), (lambda: _small((0, 1)), (1, 3)), (lambda: _small(()), (1, 3)), (_full, (1, 16))],
                         ids=["levels1", "levels01", "no_levels", "sdf_chd8bar_txt"])
def test_plan_accounting_over_groups(lib, make, Bs):
    m = make()
    h = m._h
    for Bn in Bs:
        # three groups: the prefix once, plus the hand-over's copies - two tensors (running tensor, its statistics) x three groups
        assert m.n_launches(3 * Bn, shared_x=3) == m.n_launches(3 * Bn) + 6
        assert m.n_launches(2 * Bn, shared_x=True) == m.n_launches(2 * Bn, shared_x=2) == m.n_launches(2 * Bn) + 4
        assert lib.pf_unet_workspace_bytes_cfgn(h, 3 * Bn, 3, 1) > 0
        for prepared in (0, 1):
            assert lib.pf_unet_n_launches_cfgn(h, 2 * Bn, 2, 1, prepared, prepared) == lib.pf_unet_n_launches_cfg(h, 2 * Bn, 1, prepared, prepared) > 0
            assert m.n_launches(3 * Bn, prepared=bool(prepared), shared_x=3) == lib.pf_unet_n_launches_cfgn(h, 3 * Bn, 3, 1, prepared, prepared)
        assert lib.pf_unet_workspace_bytes_cfgn(h, 2 * Bn, 2, 1) == lib.pf_unet_workspace_bytes_cfg(h, 2 * Bn, 1) > 0
    for groups, batch in ((1, 6), (4, 8), (0, 6), (-2, 6), (3, 4), (3, 2), (2, 3), (3, 0), (3, -3)):
        assert lib.pf_unet_n_launches_cfgn(h, batch, groups, 1, 0, 0) == 0
        assert lib.pf_unet_workspace_bytes_cfgn(h, batch, groups, 1) == 0
        # the forward refuses the same before it looks at a pointer or launches anything
        assert lib.pf_unet_forward_cfgn(h, FAKE, FAKE, FAKE, batch, groups, 1, None, FAKE, FAKE, 1 << 20, None) == EINVAL
        assert "guidance groups" in lib.pf_last_error().decode()
    with pytest.raises(ValueError):
        m.n_launches(4, shared_x=4)


# ---- float64 facts ----------------------------------------------------------------------------------------------------------
def test_float64_reductions():
    """On a small analytic denoiser: equal scales are single-scale guidance, (1, 1) is the conditional evaluation, second == 0 is single-scale
    guidance towards the partial condition; the second scale and the order both matter."""
    rng = np.random.default_rng(0)
    W = rng.standard_normal((D, 5))
    model = lambda x, c: 0.7 * x + np.tanh(c @ W)            # (nonlinear in c: the two orders differ in general)
    x, c, uc = rng.standard_normal((B, 1, 5)), rng.standard_normal((B, 1, D)), -np.ones((1, 1, D))
    for order in guidance_ref.ORDERS:
        for s in (0.0, 1.0, 2.5, -1.0):
            assert np.abs(guidance_ref.dual(model, x, c, uc, s, s, K, order) - guidance_ref.single(model, x, c, uc, s)).max() < 1e-12
        assert np.abs(guidance_ref.dual(model, x, c, uc, 1.0, 1.0, K, order) - model(x, c)).max() < 1e-12
        part = guidance_ref.partial(c, uc, K, order)
        assert np.abs(guidance_ref.dual(model, x, c, uc, 2.5, 0.0, K, order) - guidance_ref.single(model, x, part, uc, 2.5)).max() < 1e-12
        assert np.abs(guidance_ref.dual(model, x, c, uc, 3.0, 5.0, K, order) - guidance_ref.dual(model, x, c, uc, 3.0, 4.0, K, order)).max() > 1e-3
    assert np.abs(guidance_ref.dual(model, x, c, uc, 3.0, 5.0, K, "chd,txt") - guidance_ref.dual(model, x, c, uc, 3.0, 5.0, K, "txt,chd")).max() > 1e-3
    # the float32 step-by-step restatement of the kernel agrees with float64 to float32 rounding, and reduces to the two-way combine
    e = rng.standard_normal((3, 1000)).astype(np.float32)
    got = guidance_ref.combine3_f32(e[0], e[1], e[2], 3.0, 5.0).astype(np.float64)
    want = e[0].astype(np.float64) + 3.0 * (e[1].astype(np.float64) - e[0]) + 5.0 * (e[2].astype(np.float64) - e[1])
    e64 = e.astype(np.float64)
    big = (np.abs(e64[0]) + 3.0 * np.abs(e64[1] - e64[0]) + 5.0 * np.abs(e64[2] - e64[1])).max()       # bounds every intermediate
    assert np.abs(got - want).max() <= 5 * 2.0 ** -24 * big * (1 + 2.0 ** -20)                          # five roundings of at most half an ulp
    assert np.array_equal(guidance_ref.combine3_f32(e[0], e[1], e[1], 3.0, 5.0), guidance_ref.combine2_f32(e[0], e[1], 3.0))
