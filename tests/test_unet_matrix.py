"""The UNet plan matrix (tests/unet_matrix.py) without a GPU (-m "not gpu"): the float64 oracle pinned to the real reference at three
of the matrix's architectures (tests/golden/unet_matrix.npz, tools/make_goldens_unet_matrix.py), the range of every case's truth, and
what the library's host entry points say of every case - created, the reference's parameter table, a workspace and a launch count in
every mode - with the differences in launch count that show a case reaches the branch it is in the table for.  Absolute launch counts are
not asserted: a performance change may move them."""
import os

import numpy as np
import pytest
import torch

import unet_matrix as UM
from oracle import unet_ref
from polyffusion_amd import _lib
from polyffusion_amd.arch import unet_param_shapes

TOL = 1e-5   # tests/test_oracle_golden.py: fp32 reorder noise
CASE_FORMS, CASE_FORM_IDS = UM.case_forms()


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        from polyffusion_amd.build import build
        build(verbose=False)
    return _lib.load()


def test_case_table_is_the_one_the_gpu_module_expects():
    assert UM.CASE_IDS == ["a", "b", "c-n1", "c-n5", "d-16x8", "d-32x16", "e-b3", "e-n4", "f", "g", "h-3to1", "h-4to4", "i", "j-6x10", "j-b17"]
    assert len(set(UM.CASE_IDS)) == len(UM.CASES) and set(UM.GOLDEN_CASES) <= set(UM.CASE_IDS)
    for c in UM.CASES:
        levels = len(c.cfg.channel_multipliers)
        assert c.H % (1 << (levels - 1)) == 0 and c.W % (1 << (levels - 1)) == 0
        assert c.H * c.W <= 1536 and c.B <= 17 and c.forms[0] == UM.AUTO
        assert c.n_cond == 1 or c.cfg.d_cond % 32 == 0       # pf_unet_forward refuses anything else
        t = UM.case_inputs(c)[1]
        assert c.B < 2 or (0 in t and 999 in t)              # both ends of the schedule


@pytest.mark.parametrize("name", UM.GOLDEN_CASES)
def test_oracle_matches_the_reference_at_a_new_architecture(golden, name):
    case = UM.BY_NAME[name]
    ref = golden("unet_matrix.npz")["out_" + name]
    x, t, cond = UM.case_inputs(case)
    w = unet_ref.to_torch(UM.case_state(case))   # fp32 weights, fp32 arithmetic: the reference's own
    with torch.no_grad():
        got = unet_ref.unet_forward(w, case.cfg, torch.from_numpy(x), torch.from_numpy(t), torch.from_numpy(cond)).numpy()
    assert got.shape == ref.shape == (case.B, case.cfg.out_channels, case.H, case.W)
    e = float(np.abs(got.astype(np.float64) - ref).max())
    e64 = float(np.abs(UM.oracle_case(case)["eps"] - ref).max())
    print(f"case {name}: oracle (fp32) - reference {e:.3e}, oracle (float64) - reference {e64:.3e}")
    assert e <= TOL and e64 <= TOL


@pytest.mark.parametrize("case", UM.CASES, ids=UM.CASE_IDS)
def test_case_outputs_have_an_rms_the_absolute_tolerance_means_something_for(case):
    for group in range(3):
        o = UM.oracle_case(case, group)
        assert o["eps"].shape == (case.B, case.cfg.out_channels, case.H, case.W) and o["eps"].dtype == np.float64
        r = UM.rms(o["eps"])
        print(f"case {case.name} group {group}: rms(eps) = {r:.3f}, max |eps| = {np.abs(o['eps']).max():.3f}")
        assert 0.1 <= r <= 30.0, (case.name, group, r)
    # the further groups share x and t and differ in the condition - and in the truth
    a, b = UM.oracle_case(case, 0), UM.oracle_case(case, 1)
    assert np.array_equal(a["x"], b["x"]) and np.array_equal(a["t"], b["t"]) and not np.array_equal(a["cond"], b["cond"])
    assert float(np.abs(a["eps"] - b["eps"]).max()) > 1e-3


def _modes(m):
    return ("f32", m.split_mode)


@pytest.mark.parametrize("case,form", CASE_FORMS, ids=CASE_FORM_IDS)
def test_host_plan_facts(lib, case, form):
    m = UM.apply_form(UM.make_model(case), form)
    assert m.param_shapes() == dict(unet_param_shapes(case.cfg))
    blob = m.pack_state_dict(UM.case_state(case))
    assert blob.numel() * 4 == m.weight_bytes()
    B, nc = case.B, case.n_cond
    for mode in _modes(m):
        m.set_precision(mode)
        assert lib.pf_unet_workspace_bytes(m._h, B, nc) > 0
        plain = m.n_launches(B, nc)
        assert plain > 0 and 0 < m.n_launches(B, nc, prepared=True) < plain
        for G in (2, 3):
            assert lib.pf_unet_workspace_bytes_cfgn(m._h, G * B, G, nc) > 0
            assert lib.pf_unet_workspace_bytes_cfgn(m._h, G * B + 1, G, nc) == 0      # no whole groups
            n = m.n_launches(G * B, nc, shared_x=G)
            assert n > 0 and 0 < m.n_launches(G * B, nc, prepared=True, shared_x=G) < n
    assert lib.pf_unet_time_bias_width(m._h) > 0 and lib.pf_unet_cross_bias_width(m._h) > 0


def _launches(name, mode_index, form, **kw):
    case = UM.BY_NAME[name]
    m = UM.apply_form(UM.make_model(case), form)
    m.set_precision(_modes(m)[mode_index])
    return m.n_launches(kw.pop("batch", case.B), case.n_cond, **kw)


@pytest.mark.parametrize("name", ["e-b3", "e-n4"])
def test_case_e_reaches_the_fused_mlp_when_forced_in_the_split_mode_only(lib, name):
    """4 SpatialTransformers of two layers each: every layer's three launches (LayerNorm planes, GeGLU projection, output projection)
    become one, and the last layer's takes proj_out with it."""
    assert _launches(name, 1, UM.FUSED) < _launches(name, 1, UM.AUTO)
    assert _launches(name, 0, UM.FUSED) == _launches(name, 0, UM.AUTO)


def test_case_f_reaches_the_winograd_form_when_forced(lib):
    """(the fused Winograd conv reads the producers' tile statistics itself: the finalize launches in front of it go)"""
    assert _launches("f", 1, UM.WINO_ON) < _launches("f", 1, UM.WINO_OFF)
    assert _launches("f", 1, UM.WINO_ON) < _launches("f", 1, UM.AUTO)        # (the automatic rule keeps the direct form at this size)
    assert _launches("f", 0, UM.WINO_ON) == _launches("f", 0, UM.WINO_OFF)   # a split-mode form


def test_case_d_takes_the_key_split_attention_at_batch_one(lib):
    assert _launches("d-32x16", 1, UM.WIDE) < _launches("d-32x16", 1, UM.AUTO)            # the merging launches
    assert _launches("d-32x16", 0, UM.WIDE) == _launches("d-32x16", 0, UM.AUTO)
    assert _launches("d-16x8", 1, UM.WIDE) == _launches("d-16x8", 1, UM.AUTO)             # 128 tokens at B 3: one slice


def test_case_c_prepares_its_cross_bias_block_by_block(lib):
    """prepared=True drops the two time launches and the cross-attention mat-vecs: two grouped launches where every transformer block
    has one width (a), one launch for to_v and one per block where they differ (c)."""
    for mode in (0, 1):
        saved_a = _launches("a", mode, UM.AUTO) - _launches("a", mode, UM.AUTO, prepared=True)
        saved_c = _launches("c-n1", mode, UM.AUTO) - _launches("c-n1", mode, UM.AUTO, prepared=True)
        assert saved_c > saved_a > 0, (saved_a, saved_c)


def test_create_refuses_what_the_kernels_cannot_run(lib):
    from polyffusion_amd.unet import UNetModel
    ok = dict(in_channels=2, out_channels=2, channels=32, n_res_blocks=1, attention_levels=(1,), channel_multipliers=(1, 2), n_heads=2,
              tf_layers=1, d_cond=32, img_h=16, img_w=16)
    UNetModel(**ok)
    for change, text in ((dict(n_heads=4), "d_head 16 unsupported"), (dict(channels=48), "channels must be a multiple of 32"),
                         (dict(img_w=15), "image size must be divisible by 2"), (dict(img_h=6, channel_multipliers=(1, 2, 2)), "image size must be divisible by 2"),
                         (dict(out_channels=5), "out_channels must be 1..4"), (dict(d_cond=6), "bad attention config")):
        with pytest.raises(RuntimeError, match=text):
            UNetModel(**dict(ok, **change))
