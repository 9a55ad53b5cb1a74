"""The UNet plan on the MI355X against the float64 oracle (oracle/unet_ref.py, pinned to the real reference at three of these
architectures by tests/test_unet_matrix.py) at the architectures, image shapes, batches and plan options of tests/unet_matrix.py - the
table there gives every case's configuration.  What each case reaches in run() / run_st() (csrc/unet.hip) and in the shared emitters
(csrc/unet_blocks.hip), and its worst observed max-abs-diff against the oracle over its plan-option forms (MI355X; f32 / bf16x3 / f16x3):

  a        two transformer layers at d_head 32 (the t0 / t1 / t2 rotation of run_st), two ResBlocks per level   2.8e-06 / 4.3e-05 / 2.3e-06
  b        the same with n_cond 3: the general cross-attention inside the rotation                               2.8e-06 / 4.4e-05 / 1.6e-06
  c-n1     transformer blocks of widths 32 and 64 (the per-block cross mat-vecs), attention at level 0,
           planes at C = 64 in the split modes, 32x16                                                            2.9e-06 / 4.6e-05 / 2.2e-06
  c-n5     the same with n_cond 5                                                                                2.6e-06 / 4.1e-05 / 2.0e-06
  d-16x8   one level, planes with two layers (last_planes for the second only), d_cond 8; attn_wide forced
           where the 256-query form does not exist (128 tokens)                                                  2.6e-06 / 3.0e-05 / 2.2e-06
  d-32x16  512 tokens at B 1: the key-split attention with its merging launch, and attn_wide=True beside it       3.4e-06 / 4.1e-05 / 3.0e-06
  e-b3     C = 256 at 128 tokens: the fused MLP forced on (plain launch, then the launch with proj_out and
           the tile statistics) and the chain                                                                    4.8e-06 / 4.3e-05 / 2.9e-06
  e-n4     the same at B 1 with n_cond 4                                                                         5.3e-06 / 4.2e-05 / 2.7e-06
  f        Winograd forced on / off at a 32x48 level, 384 tokens of planes attention below it                    3.7e-06 / 4.2e-05 / 3.2e-06
  g        no attention level: only the middle block looks at the condition                                      2.0e-06 / 2.7e-05 / 2.1e-06
  h-3to1   stem cin 3 (statistics from stats_pass), head cout 1, d_cond 4, B 5                                   2.8e-06 / 3.9e-05 / 1.9e-06
  h-4to4   stem cin 4, head cout 4, B 1, n_cond 2                                                                2.5e-06 / 3.7e-05 / 1.6e-06
  i        three levels with a repeated multiplier, two ResBlocks, 64 tokens at the deepest level                3.2e-06 / 4.7e-05 / 1.9e-06
  j-6x10   60 pixels, 15 tokens: every tile wider than the image; n_cond 2                                       2.1e-06 / 5.0e-05 / 1.7e-06
  j-b17    8x8, 16 tokens, batch 17                                                                              2.8e-06 / 4.0e-05 / 2.0e-06

Per case, form and mode: eps against the float64 oracle at the project's own bars - f32 1e-4 (tests/test_gpu_unet.py), bf16x3 5e-4
(tests/test_gpu_bf16x3.py), f16x3 1e-4 * max(1, |ref|max) (tests/test_gpu_f16x3.py), all under the 1e-3 contract of BASELINE.json -
finite, and the same bits twice.  In case e the forced fused MLP must give the bits of the chain.

Worst observed over all cases, forms and guidance groups (MI355X):  f32 5.9e-06 (e-b3, second group)   bf16x3 5.0e-05 (j-6x10)
f16x3 3.2e-06 (f, conv_wino on).  No case comes within a factor of ten of its bar.

Then the forms of the forward in bf16x3 and f32 (prepared tables: the same bits; two and three guidance groups: each group against its
own oracle, and against the plain forward of the stacked batch at 2e-5; batch composition at 2e-5 - both measured 0 at these shapes;
the tracked plan, whose absmax measured 9.7 ... 22.3 against max |eps| 1.9 ... 2.6), and the raw C calls: the workspace the plan asks
for inside guard bytes, one byte less refused, the call- and create-time refusals."""
import ctypes

import numpy as np
import pytest
import torch

import unet_matrix as UM
from polyffusion_amd import _lib

pytestmark = pytest.mark.gpu

MODES = [("f32", None), ("bf16x3", None), ("f16x3", "f16")]
FORM_MODES = [("bf16x3", None), ("f32", None)]
ROUNDING = 2e-5   # tile-choice rounding: test_batch_composition_independence of tests/test_gpu_unet.py
CASE_FORMS, CASE_FORM_IDS = UM.case_forms()
_models = {}


def bar(mode, ref) -> float:
    return {"f32": 1e-4, "bf16x3": 5e-4, "f16x3": 1e-4 * max(1.0, float(np.abs(ref).max()))}[mode]


def _model(case, mode, x3, form=UM.AUTO):
    """One handle per (net, image size, weights, library), shared by the tests; mode and plan options are set per use."""
    key = (case.cfg, case.H, case.W, case.seed, x3)
    if key not in _models:
        _models[key] = UM.make_model(case, x3).load_state_dict(UM.case_state(case))
    m = _models[key]
    if m._amax is not None:
        m.track_absmax(False)
    return UM.apply_form(m.set_precision(mode), form)


def _dev(o, *names):
    return tuple(torch.tensor(o[n]).cuda() for n in names)   # (a copy: the oracle's arrays are read-only)


def _err(got, ref):
    return float((got.detach().cpu().double() - torch.tensor(ref)).abs().max())


def _stacked(case, G):
    """x [B], t [G*B], cond [G*B] of a shared_x evaluation (equal t per group) and the oracles of its groups"""
    os_ = [UM.oracle_case(case, g) for g in range(G)]
    x, t = _dev(os_[0], "x", "t")
    cond = torch.cat([_dev(o, "cond")[0] for o in os_])
    return x, t.repeat(G), cond, os_


@pytest.mark.parametrize("mode,x3", MODES)
@pytest.mark.parametrize("case,form", CASE_FORMS, ids=CASE_FORM_IDS)
def test_case_matches_the_float64_oracle(case, form, mode, x3):
    o = UM.oracle_case(case)
    m = _model(case, mode, x3, form)
    x, t, cond = _dev(o, "x", "t", "cond")
    eps = m(x, t, cond).clone()
    e = _err(eps, o["eps"])
    print(f"case {case.name} {UM.form_id(form)} {mode}: max-abs-diff {e:.3e} (bar {bar(mode, o['eps']):.1e})")
    assert eps.shape == o["eps"].shape and bool(torch.isfinite(eps).all())
    assert torch.equal(m(x, t, cond), eps)
    assert e < bar(mode, o["eps"]), e


@pytest.mark.parametrize("mode,x3", MODES)
@pytest.mark.parametrize("name", ["e-b3", "e-n4"])
def test_forced_fused_mlp_gives_the_bits_of_the_chain(name, mode, x3):
    """csrc/mlp_fused_bf3.hip: bit-identical to LayerNorm planes + GeGLU GEMM + FF-out GEMM (+ proj_out)"""
    case = UM.BY_NAME[name]
    x, t, cond = _dev(UM.oracle_case(case), "x", "t", "cond")
    chain = _model(case, mode, x3, UM.AUTO)(x, t, cond).clone()
    fused = _model(case, mode, x3, UM.FUSED)(x, t, cond)
    if mode != "f32":
        m = _model(case, mode, x3)
        assert UM.apply_form(m, UM.FUSED).n_launches(case.B, case.n_cond) < UM.apply_form(m, UM.AUTO).n_launches(case.B, case.n_cond)
    assert torch.equal(fused, chain), float((fused - chain).abs().max())


def test_forced_wide_attention_runs_where_the_form_does_not_exist():
    """128 tokens: attn_wide=True leaves the level on the 128-query kernel - the bits of the automatic plan."""
    case = UM.BY_NAME["d-16x8"]
    x, t, cond = _dev(UM.oracle_case(case), "x", "t", "cond")
    auto = _model(case, "bf16x3", None, UM.AUTO)(x, t, cond).clone()
    assert torch.equal(_model(case, "bf16x3", None, UM.WIDE)(x, t, cond), auto)


# ---- forms of the forward ----
FORMS_CASES = [("a", UM.AUTO), ("c-n1", UM.AUTO), ("c-n5", UM.AUTO), ("d-16x8", UM.AUTO), ("e-b3", UM.FUSED), ("g", UM.AUTO)]
FORMS_IDS = [n for n, _ in FORMS_CASES]


@pytest.mark.parametrize("mode,x3", FORM_MODES)
@pytest.mark.parametrize("name,form", FORMS_CASES, ids=FORMS_IDS)
def test_prepared_tables_give_the_same_bits(name, form, mode, x3):
    case = UM.BY_NAME[name]
    o = UM.oracle_case(case)
    m = _model(case, mode, x3, form)
    x, t, cond = _dev(o, "x", "t", "cond")
    plain = m(x, t, cond).clone()
    table = m.prepare_time(1000)
    cross = m.prepare_cond(cond)
    assert (cross is None) == (case.n_cond > 1)
    assert torch.equal(m(x, t, cond, time_table=table, cross_bias=cross, check_t=True), plain)
    assert torch.equal(m(x, t, cond, time_table=table), plain)
    if cross is not None:
        assert cross.shape == (case.B, m._lib.pf_unet_cross_bias_width(m._h))
        assert torch.equal(m(x, t, cond, cross_bias=cross), plain)
    assert _err(plain, o["eps"]) < bar(mode, o["eps"])


@pytest.mark.parametrize("mode,x3", FORM_MODES)
@pytest.mark.parametrize("G", [2, 3])
@pytest.mark.parametrize("name,form", FORMS_CASES, ids=FORMS_IDS)
def test_guidance_groups_share_the_prefix_and_nothing_else(name, form, G, mode, x3):
    case = UM.BY_NAME[name]
    m = _model(case, mode, x3, form)
    x, t, cond, os_ = _stacked(case, G)
    B = case.B
    got = m(x, t, cond, shared_x=G, check_t=True).clone()
    assert got.shape[0] == G * B and bool(torch.isfinite(got).all())
    errs = [_err(got[g * B:(g + 1) * B], os_[g]["eps"]) for g in range(G)]
    stacked = m(x.repeat(G, 1, 1, 1), t, cond)
    d = float((got - stacked).abs().max())
    print(f"case {name} G={G} {mode}: per group {['%.3e' % e for e in errs]}, shared - stacked {d:.3e}")
    for g in range(G):
        assert errs[g] < bar(mode, os_[g]["eps"]), (g, errs)
    assert d < ROUNDING, d
    for g in range(1, G):   # the groups differ (in case g: through the middle block alone)
        assert float((got[g * B:(g + 1) * B] - got[:B]).abs().max()) > 1e-3
    # with both prepared tables: the same bits
    cross = m.prepare_cond(cond)
    assert torch.equal(m(x, t, cond, shared_x=G, time_table=m.prepare_time(1000), cross_bias=cross), got)


@pytest.mark.parametrize("mode,x3", FORM_MODES)
@pytest.mark.parametrize("name,form", [("b", UM.AUTO), ("e-b3", UM.FUSED), ("e-b3", UM.AUTO)], ids=["b", "e-b3-fused", "e-b3-chain"])
def test_batch_composition(name, form, mode, x3):
    case = UM.BY_NAME[name]
    o = UM.oracle_case(case)
    m = _model(case, mode, x3, form)
    x, t, cond = _dev(o, "x", "t", "cond")
    full = m(x, t, cond).clone()
    for i in range(case.B):
        one = m(x[i:i + 1].contiguous(), t[i:i + 1], cond[i:i + 1].contiguous())
        d = float((one[0] - full[i]).abs().max())
        print(f"case {name} {UM.form_id(form)} {mode}: sample {i} alone - in the batch {d:.3e}")
        assert d < ROUNDING, (i, d)


@pytest.mark.parametrize("mode,x3", FORM_MODES)
@pytest.mark.parametrize("name,form", FORMS_CASES, ids=FORMS_IDS)
def test_tracked_plan(name, form, mode, x3):
    """track_absmax(True): the plan runs chains in place of fused launches and max-combines every stored |value|"""
    case = UM.BY_NAME[name]
    o = UM.oracle_case(case)
    m = _model(case, mode, x3, form)
    x, t, cond = _dev(o, "x", "t", "cond")
    try:
        m.track_absmax(True)
        eps = m(x, t, cond).clone()
        amax = m.read_absmax()
    finally:
        m.track_absmax(False)
    e, top = _err(eps, o["eps"]), float(eps.abs().max())
    print(f"case {name} {mode}: tracked max-abs-diff {e:.3e}, absmax {amax:.4f}, max |eps| {top:.4f}")
    assert e < bar(mode, o["eps"])
    assert np.isfinite(amax) and amax >= top      # a maximum over every stored tensor: no upper side


# ---- the raw C calls ----
def _canaried(nbytes):
    """(buffer, pointer to `nbytes` bytes inside it with 64 KiB of pattern on either side, check)"""
    pad, pattern = 64 * 1024, 0xA5
    buf = torch.full((pad + nbytes + pad,), pattern, dtype=torch.uint8, device="cuda")
    return buf, buf.data_ptr() + pad, (lambda: bool((buf[:pad] == pattern).all()) and bool((buf[pad + nbytes:] == pattern).all()))


@pytest.mark.parametrize("mode,x3", MODES)
@pytest.mark.parametrize("name,form", [("c-n5", UM.AUTO), ("d-32x16", UM.AUTO), ("e-b3", UM.FUSED)], ids=["c-n5", "d-32x16", "e-b3"])
def test_calls_stay_inside_the_workspace_they_asked_for(name, form, mode, x3):
    case = UM.BY_NAME[name]
    m = _model(case, mode, x3, form)
    lib, B, nc = m._lib, case.B, case.n_cond
    stream = _lib.current_stream()

    def run(call, nb, rows):
        out = torch.full((rows, case.cfg.out_channels, case.H, case.W), float("nan"), device="cuda")
        buf, ws, intact = _canaried(nb)
        assert nb > 0 and call(out, ws, nb - 1) == -1 and "workspace too small" in lib.pf_last_error().decode()
        torch.cuda.synchronize()
        assert bool(torch.isnan(out).all()) and intact(), "a refused call launched something"
        _lib.check(call(out, ws, nb), "pf_unet_forward", lib)
        torch.cuda.synchronize()
        assert intact(), "the forward wrote outside its workspace"
        return out

    o = UM.oracle_case(case)
    x, t, cond = _dev(o, "x", "t", "cond")
    nb = int(lib.pf_unet_workspace_bytes(m._h, B, nc))
    eps = run(lambda out, ws, n: lib.pf_unet_forward(m._h, x.data_ptr(), t.data_ptr(), cond.data_ptr(), B, nc, out.data_ptr(), ws, n, stream), nb, B)
    assert _err(eps, o["eps"]) < bar(mode, o["eps"])

    x, t2, cond2, os_ = _stacked(case, 2)
    nb = int(lib.pf_unet_workspace_bytes_cfgn(m._h, 2 * B, 2, nc))
    eps2 = run(lambda out, ws, n: lib.pf_unet_forward_cfgn(m._h, x.data_ptr(), t2.data_ptr(), cond2.data_ptr(), 2 * B, 2, nc, None, out.data_ptr(),
                                                          ws, n, stream), nb, 2 * B)
    for g in range(2):
        assert _err(eps2[g * B:(g + 1) * B], os_[g]["eps"]) < bar(mode, os_[g]["eps"])


def test_calls_the_plan_cannot_run_are_refused_before_anything_is_launched():
    """Each refusal returns -1 with its message and leaves the (NaN-filled) output untouched."""
    d, b = UM.BY_NAME["d-16x8"], UM.BY_NAME["b"]
    md, mb = _model(d, "bf16x3", None), _model(b, "bf16x3", None)
    lib, stream = md._lib, _lib.current_stream()
    out = torch.full((8 * 2 * 16 * 16,), float("nan"), device="cuda")
    x = torch.randn(8 * 2 * 16 * 16, device="cuda")
    cond = torch.randn(8 * 8 * 32, device="cuda")
    t = torch.zeros(8, dtype=torch.int64, device="cuda")
    ws = torch.empty(max(int(lib.pf_unet_workspace_bytes(md._h, 6, 2)), int(lib.pf_unet_workspace_bytes_cfgn(md._h, 6, 2, 1)),
                         int(lib.pf_unet_workspace_bytes(mb._h, 2, 3))), dtype=torch.uint8, device="cuda")
    assert ws.numel() > 0

    def untouched():
        torch.cuda.synchronize()
        return bool(torch.isnan(out).all())

    ptrs = (x.data_ptr(), t.data_ptr(), cond.data_ptr())
    tail = (out.data_ptr(), ws.data_ptr(), ws.numel(), stream)
    # several condition tokens at a d_cond the general cross-attention cannot read (d_cond 8)
    assert lib.pf_unet_forward(md._h, *ptrs, 3, 2, *tail) == -1 and "n_cond > 1 needs d_cond % 32 == 0" in lib.pf_last_error().decode()
    assert untouched()
    # five rows are not two groups of one size
    assert lib.pf_unet_workspace_bytes_cfgn(md._h, 5, 2, 1) == 0
    assert lib.pf_unet_forward_cfgn(md._h, *ptrs, 5, 2, 1, None, *tail) == -1
    assert "2 or 3 guidance groups of one size (got 5 rows, 2 groups)" in lib.pf_last_error().decode()
    assert untouched()
    # a collapsed cross-attention bias with three condition tokens
    prep = _lib.UNetPrepared()
    prep.cross_bias = x.data_ptr()
    assert lib.pf_unet_forward_prepared(mb._h, *ptrs, 2, 3, ctypes.byref(prep), *tail) == -1
    assert "the collapsed cross-attention bias exists only for n_cond == 1" in lib.pf_last_error().decode()
    assert untouched()
    with pytest.raises(RuntimeError, match="n_cond > 1 needs d_cond"):
        md(torch.zeros(3, 2, 16, 8).cuda(), t[:3], torch.zeros(3, 2, 8).cuda())
    # the calls beside them run
    assert lib.pf_unet_forward_cfgn(md._h, *ptrs, 6, 2, 1, None, *tail) == 0 and lib.pf_unet_forward(mb._h, *ptrs, 2, 3, *tail) == 0
    assert not untouched()


def test_configurations_the_kernels_cannot_run_are_refused_at_create():
    lib = _lib.load()

    def create(**change):
        kw = dict(in_channels=2, out_channels=2, channels=32, n_res_blocks=1, attention_levels=(1,), channel_multipliers=(1, 2), n_heads=2,
                  tf_layers=1, d_cond=32, img_h=16, img_w=16)
        kw.update(change)
        c = _lib.UNetCfg()
        c.in_channels, c.out_channels, c.channels, c.n_res_blocks = kw["in_channels"], kw["out_channels"], kw["channels"], kw["n_res_blocks"]
        c.n_attention_levels, c.n_levels = len(kw["attention_levels"]), len(kw["channel_multipliers"])
        for i, v in enumerate(kw["attention_levels"]):
            c.attention_levels[i] = v
        for i, v in enumerate(kw["channel_multipliers"]):
            c.channel_multipliers[i] = v
        c.n_heads, c.tf_layers, c.d_cond, c.img_h, c.img_w = kw["n_heads"], kw["tf_layers"], kw["d_cond"], kw["img_h"], kw["img_w"]
        h = ctypes.c_void_p()
        rc = lib.pf_unet_create(ctypes.byref(c), ctypes.byref(h))
        if h:
            lib.pf_unet_destroy(h)
        return rc, lib.pf_last_error().decode()

    assert create()[0] == 0
    for change, text in ((dict(n_heads=4), "d_head 16 unsupported (32 or 64)"),            # level 1: 64 / 4
                         (dict(channels=48), "channels must be a multiple of 32"),
                         (dict(img_h=16, img_w=15), "image size must be divisible by 2^(levels-1)"),
                         (dict(img_h=6, img_w=8, channel_multipliers=(1, 2, 2)), "image size must be divisible by 2^(levels-1)")):
        rc, msg = create(**change)
        assert rc == -1 and text in msg, (change, rc, msg)
    assert create(img_h=6, img_w=10)[0] == 0 and create(n_heads=1)[0] == 0
