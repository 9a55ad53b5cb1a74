"""oracle/autoencoder_ref.py (the float64 restatement of the first-stage autoencoder) pinned to tests/golden/autoencoder.npz, and the
case table that tests/test_gpu_autoencoder_oracle.py runs on the GPU (-m "not gpu": nothing here needs one).

The goldens are float32 runs of the real reference; the float64 oracle differs from them by the reference's own roundoff.  Measured
max-abs-diff per array (CPU, float64 oracle against the fixture):

    small_mean     1.06e-06      clamp_mean     1.06e-06      full_mean     1.49e-06
    small_log_var  1.38e-06      clamp_log_var  4.33e-06      full_log_var  1.85e-06
    small_z        3.15e-06                                   full_dec      2.76e-06
    small_dec      1.51e-06
    small_forward  2.34e-06

Each array is asserted at 10x its measurement (PIN), and every bound is itself held under 1e-4, a tenth of the project's 1e-3 contract:
a restatement that needed more would be a different model, not a noisier one.

CASES is the table of configurations, seeds and shapes the GPU module checks against this oracle.  Weights are
synth_autoencoder_state(cfg, seed), inputs and noise come from numpy's PCG64(seed + 1) / PCG64(seed + 2).  For every case each oracle
output (mean, log_var, z, decode(z)) has its rms in [0.1, 30] - the condition tools/make_goldens_autoencoder.py puts on the fixture,
and what gives an absolute tolerance of 1e-3 on them a meaning."""
import os
from functools import lru_cache
from typing import NamedTuple

import numpy as np
import pytest
import torch

from oracle import autoencoder_ref as R
from polyffusion_amd.autoencoder import AutoencoderConfig
from polyffusion_amd.weights import synth_autoencoder_state

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = np.load(os.path.join(REPO, "tests", "golden", "autoencoder.npz"))
SMALL = AutoencoderConfig(in_channels=3, out_channels=3, channels=32, channel_multipliers=(1, 2), n_resnet_blocks=1, z_channels=4,
                          emb_channels=4)
FULL = AutoencoderConfig()

# 10x the measured difference of the docstring, per array
PIN = {"small_mean": 1.1e-5, "small_log_var": 1.4e-5, "small_z": 3.2e-5, "small_dec": 1.6e-5, "small_forward": 2.4e-5,
       "clamp_mean": 1.1e-5, "clamp_log_var": 4.4e-5, "full_mean": 1.5e-5, "full_log_var": 1.9e-5, "full_dec": 2.8e-5}
PIN_CAP = 1e-4


class Case(NamedTuple):
    name: str
    cfg: AutoencoderConfig
    seed: int
    B: int
    H: int
    W: int


def _cfg(cin, cout, channels, mult, blocks, z, emb):
    return AutoencoderConfig(in_channels=cin, out_channels=cout, channels=channels, channel_multipliers=mult, n_resnet_blocks=blocks,
                             z_channels=z, emb_channels=emb)


CFG_A = _cfg(1, 1, 32, (1,), 1, 1, 1)         # one level (f = 1), Z2 = 2, E = 1, stem cin 1, head cout 1
CFG_B = _cfg(2, 2, 32, (1, 2), 1, 2, 3)       # Z2 = 4, emb != z in both 1x1s
CFG_C = _cfg(4, 4, 32, (1, 3), 1, 3, 2)       # Z2 = 6, top width 96
CFG_D = _cfg(2, 3, 64, (1, 1, 2), 2, 4, 4)    # the stem's register-weight kernel (cin 2 -> 64), three levels, two blocks
CFG_E = _cfg(3, 3, 32, (2, 1), 1, 4, 4)       # widths that decrease with depth
# The split modes split a 3x3 conv's K four ways (conv_splitk_ws_bytes) only from 384 input channels - twelve 32-channel chunks - on a
# grid of at most a quarter of the CUs.  No net above is that wide, the full one (top width 256) included: without this case the split
# never runs under this model.  One level at width 384 puts such convs at M = 64 rows, the fewest the attention allows: conv2 of the
# 128 -> 384 block with the fused 1x1 shortcut, and the 384 -> 384 convs of the mid blocks and of the decoder
# (test_only_case_i_splits_k checks which layers split, without a GPU).
CFG_I = _cfg(3, 3, 128, (3,), 1, 4, 4)
CASES = [
    Case("a", CFG_A, 1, 1, 8, 8),
    Case("b", CFG_B, 2, 2, 16, 16),
    Case("c", CFG_C, 3, 5, 16, 32),
    Case("d", CFG_D, 4, 3, 64, 64),
    Case("e", CFG_E, 5, 1, 16, 16),
    Case("f-square", SMALL, 6, 1, 64, 64),    # 1024 tokens, 32x32
    Case("f-strip", SMALL, 6, 1, 32, 128),    # 1024 tokens, 16x64
    Case("g-b1", SMALL, 7, 1, 32, 16),
    Case("g-b16", SMALL, 7, 16, 32, 16),
    Case("g-b17", SMALL, 7, 17, 32, 16),
    Case("h", FULL, 8, 2, 64, 64),            # four levels at a size the fixture does not hold
    Case("i", CFG_I, 9, 1, 8, 8),             # split-K at M = 64, with and without the fused shortcut
]
CASE_IDS = [c.name for c in CASES]


def randn(seed, shape):
    return np.random.Generator(np.random.PCG64(seed)).standard_normal(shape).astype(np.float32)


def rms(a) -> float:
    return float(np.sqrt(np.mean(np.square(np.asarray(a, dtype=np.float64)))))


def case_inputs(case):
    """(state, x, noise) of a case as float32 numpy: what the GPU gets."""
    f = case.cfg.downscale
    state = synth_autoencoder_state(case.cfg, case.seed)
    x = randn(case.seed + 1, (case.B, case.cfg.in_channels, case.H, case.W))
    noise = randn(case.seed + 2, (case.B, case.cfg.emb_channels, case.H // f, case.W // f))
    return state, x, noise


@lru_cache(maxsize=None)
def oracle_case(case):
    """The float64 truth of a case, computed once per process and shared: x, noise, mean, log_var, z = sample(noise) and dec =
    decode(z rounded to float32 - the tensor the GPU decoder is handed).  Callers must leave the arrays unchanged."""
    state, x, noise = case_inputs(case)
    w = R.to_torch(state, torch.float64)
    with torch.no_grad():
        mean, log_var = R.encode(w, case.cfg, torch.from_numpy(x).double())
        z = R.sample(mean, log_var, torch.from_numpy(noise).double(), 1.0)
        z32 = z.float()
        dec = R.decode(w, case.cfg, z32.double(), 1.0)
    out = {"x": x, "noise": noise, "mean": mean.numpy(), "log_var": log_var.numpy(), "z": z.numpy(), "z32": z32.numpy(), "dec": dec.numpy()}
    for v in out.values():
        v.setflags(write=False)
    return out


def _t(name):
    return torch.from_numpy(G[name]).double()


def _pin(got, name):
    e = float((got - _t(name)).abs().max())
    print(f"{name}: oracle - golden max-abs-diff {e:.3e} (bound {PIN[name]:.1e})")
    assert PIN[name] <= PIN_CAP
    assert e < PIN[name], (name, e)


def clamp_state(cfg):
    """tools/make_goldens_autoencoder.py clamp_state: the first / second log_var channel's quant_conv bias shifted by +20 / -30."""
    st = synth_autoencoder_state(cfg, 0)
    b = st["quant_conv.bias"].copy()
    b[cfg.emb_channels + 0] += np.float32(20.0)
    b[cfg.emb_channels + 1] += np.float32(-30.0)
    st["quant_conv.bias"] = b
    return st


def test_every_fixture_array_has_a_bound_under_the_cap():
    arrays = {k for k in G.files if k.split("_")[0] in ("small", "clamp", "full")} - {"small_x", "small_noise", "full_x_seed"}
    assert arrays == set(PIN) and max(PIN.values()) <= PIN_CAP


@torch.no_grad()
def test_oracle_matches_the_small_fixture():
    w = R.to_torch(synth_autoencoder_state(SMALL, 0), torch.float64)
    x, noise = _t("small_x"), _t("small_noise")
    mean, log_var = R.encode(w, SMALL, x)
    _pin(mean, "small_mean")
    _pin(log_var, "small_log_var")
    _pin(R.sample(mean, log_var, noise, 1.0), "small_z")
    _pin(R.decode(w, SMALL, _t("small_z"), 1.0), "small_dec")
    fwd, m2, lv2 = R.forward(w, SMALL, x, noise)
    _pin(fwd, "small_forward")
    assert torch.equal(m2, mean) and torch.equal(lv2, log_var)
    # the scale: sample multiplies by it, decode divides by it
    s = 0.18215
    assert torch.allclose(R.sample(mean, log_var, noise, s), s * R.sample(mean, log_var, noise, 1.0), rtol=1e-14, atol=0)
    assert float((R.decode(w, SMALL, s * _t("small_z"), s) - _t("small_dec")).abs().max()) < PIN["small_dec"]


@torch.no_grad()
def test_oracle_matches_the_clamp_fixture():
    w = R.to_torch(clamp_state(SMALL), torch.float64)
    mean, log_var = R.encode(w, SMALL, _t("small_x"))
    _pin(mean, "clamp_mean")
    _pin(log_var, "clamp_log_var")
    ref = torch.from_numpy(G["clamp_log_var"])
    lo, hi = ref == -30.0, ref == 20.0
    assert int(lo.sum()) >= ref.numel() // 100 and int(hi.sum()) >= ref.numel() // 100
    assert bool((log_var[lo] == -30.0).all()) and bool((log_var[hi] == 20.0).all())
    assert float(log_var.min()) >= -30.0 and float(log_var.max()) <= 20.0


@torch.no_grad()
def test_oracle_matches_the_full_fixture():
    w = R.to_torch(synth_autoencoder_state(FULL, 0), torch.float64)
    x = torch.from_numpy(randn(int(G["full_x_seed"]), (1, 3, 128, 128))).double()
    mean, log_var = R.encode(w, FULL, x)
    _pin(mean, "full_mean")
    _pin(log_var, "full_log_var")
    _pin(R.decode(w, FULL, _t("full_mean"), 1.0), "full_dec")


def test_only_case_i_splits_k():
    """What the plan asks of pf_conv_splitk_ws_bytes for a ResnetBlock conv (3x3, stride 1, split mode) at a case's latent size: four
    fp32 partial sums of the output for case i, nothing for the 3x3 convs of every other case, the full net's included."""
    import ctypes

    from polyffusion_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        from polyffusion_amd.build import build
        build(verbose=False)
    lib = _lib.load()

    def ws_bytes(B, h, w, cin, cout):
        a = _lib.ConvArgs()
        a.c0, a.batch, a.hin, a.win, a.ks, a.stride, a.n, a.ld_out, a.precision = cin, B, h, w, 3, 1, cout, cout, 1
        return int(lib.pf_conv_splitk_ws_bytes(ctypes.byref(a)))

    for c in CASES:
        f = c.cfg.downscale
        widths = sorted({c.cfg.channels * m for m in c.cfg.channel_multipliers} | {c.cfg.channels})
        got = {(ci, co): ws_bytes(c.B, c.H // f, c.W // f, ci, co) for ci in widths for co in widths}
        if c.name == "i":
            assert got[(384, 384)] == 4 * 64 * 384 * 4 and got[(128, 384)] == 0, got   # conv2 (K = 9 * 384) splits, conv1 of 128 -> 384 does not
        else:
            assert not any(got.values()), (c.name, got)


def test_case_table_is_the_one_the_gpu_module_expects():
    assert CASE_IDS == ["a", "b", "c", "d", "e", "f-square", "f-strip", "g-b1", "g-b16", "g-b17", "h", "i"] and len(set(CASE_IDS)) == len(CASES)
    for c in CASES:
        f = c.cfg.downscale
        assert c.H % f == 0 and c.W % f == 0
        tokens = (c.H // f) * (c.W // f)
        assert tokens % 64 == 0 and tokens <= 1024, c


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_case_outputs_have_an_rms_the_absolute_tolerance_means_something_for(case):
    o = oracle_case(case)
    f, cfg = case.cfg.downscale, case.cfg
    assert o["mean"].shape == o["log_var"].shape == o["z"].shape == (case.B, cfg.emb_channels, case.H // f, case.W // f)
    assert o["dec"].shape == (case.B, cfg.out_channels, case.H, case.W)
    for k in ("mean", "log_var", "z", "dec"):
        r = rms(o[k])
        print(f"case {case.name}: rms({k}) = {r:.3f}")
        assert 0.1 <= r <= 30.0, (case.name, k, r)
    assert float(o["log_var"].min()) > -30.0 and float(o["log_var"].max()) < 20.0   # (the clamp has its own fixture)
