"""The first-stage autoencoder on the MI355X against the float64 oracle (oracle/autoencoder_ref.py, pinned to the reference's golden by
tests/test_oracle_autoencoder.py) at the configurations and shapes the golden does not hold.  The case table lives in
tests/test_oracle_autoencoder.py (CASES); what each case reaches:

  a  32, (1,), 1/1/1/1, B 1, 8x8          one level (no DownSample / UpSample), ae_tail<2>, E = 1, stem cin 1, head cout 1
  b  32, (1, 2), 2/2/2/3, B 2, 16x16      ae_tail<4>, emb != z: quant_conv [2E][2Z] and post_quant_conv [Z][E] are not square
  c  32, (1, 3), 4/4/3/2, B 5, 16x32      ae_tail<6>, C = 96 (N padded to 128, three channels per group, attention at d = 96, q|k|v at N = 288);
                                          latent 8x16: ae_tail's tile half empty in H
  d  64, (1, 1, 2), 2 blocks, 2/3/4/4     the stem's register-weight kernel with this model's GroupNorm, three levels, head cout 3
  e  32, (2, 1), 3/3/4/4, B 1, 16x16      nin_shortcut narrowing in the encoder and widening in the decoder
  f  the small net, B 1, 64x64 / 32x128   1024 attention tokens, latent 32x32 and 16x64 (four 16x16 tiles of ae_tail, square and strip)
  g  the small net, B 1 / 16 / 17, 32x16  latent 16x8: ae_tail's tile half empty in W; batch edges
  h  the full net, B 2, 64x64             four levels at a size and batch the golden does not hold (latent 8x8: the tile partly empty in H and W)
  i  128, (3,), 3/3/4/4, B 1, 8x8         the only net wide enough for the split modes' split-K (384 input channels): at M = 64, in conv2 of
                                          128 -> 384 with the fused shortcut and in the 384 -> 384 convs; attention at d = 384

Every case runs in f32, bf16x3 and f16x3 and checks mean, log_var, z and decode (of the oracle's z) at max-abs-diff < 1e-3, the project's
standing contract on outputs whose rms the oracle test keeps in [0.1, 30]; encode_sample and decode must give the same bits twice.

Worst observed max-abs-diff over all cases and outputs (MI355X):  f32 8.2e-06 (h, decode)   bf16x3 4.4e-05 (h, decode)   f16x3 4.3e-06 (d, decode)

Then, through the raw C calls: the workspace canaries away from B = 1 square and with split-K, NULL outputs of pf_autoenc_encode, the call- and
create-time refusals, and pf_gaussian_sample alone against float64 with a per-element bound."""
import ctypes

import numpy as np
import pytest
import torch

from polyffusion_amd import _lib
from polyffusion_amd.autoencoder import Autoencoder, AutoencoderConfig
from test_oracle_autoencoder import CASES, CASE_IDS, case_inputs, oracle_case

pytestmark = pytest.mark.gpu

MODES = [("f32", None), ("bf16x3", None), ("f16x3", "f16")]
TOL = 1e-3
_models = {}
BY_NAME = {c.name: c for c in CASES}


def _model(case, mode, x3):
    """One handle per (net, weights, library), shared by the tests; the mode is set per use."""
    key = (case.cfg, case.seed, x3)
    if key not in _models:
        _models[key] = Autoencoder(case.cfg, x3=x3).load_state_dict(case_inputs(case)[0])
    return _models[key].set_precision(mode)


def _err(got, ref):
    return float((got.detach().cpu().double() - torch.tensor(ref)).abs().max())   # (a copy: the oracle's arrays are read-only)


@pytest.mark.parametrize("mode,x3", MODES)
@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_case_matches_the_float64_oracle(case, mode, x3):
    o = oracle_case(case)
    u = _model(case, mode, x3)
    x, noise = torch.tensor(o["x"]).cuda(), torch.tensor(o["noise"]).cuda()
    z, post = u.encode_sample(x, noise=noise)
    dec = u.decode(torch.tensor(o["z32"]).cuda())
    errs = {"mean": _err(post.mean, o["mean"]), "log_var": _err(post.log_var, o["log_var"]), "z": _err(z, o["z"]), "dec": _err(dec, o["dec"])}
    print(f"case {case.name} {mode}: " + "  ".join(f"{k} {v:.3e}" for k, v in errs.items()) + f"  worst {max(errs.values()):.3e}")
    assert z.shape == o["z"].shape and dec.shape == o["dec"].shape
    # the same bits twice, and from the separate calls
    z2, post2 = u.encode_sample(x, noise=noise)
    assert torch.equal(z2, z) and torch.equal(post2.mean, post.mean) and torch.equal(post2.log_var, post.log_var)
    assert torch.equal(u.decode(torch.tensor(o["z32"]).cuda()), dec)
    post3 = u.encode(x)
    assert torch.equal(post3.mean, post.mean) and torch.equal(post3.log_var, post.log_var) and torch.equal(post3.sample(noise), z)
    assert max(errs.values()) < TOL, errs


# ---- ABI-level checks through the raw calls ----
def _canaried(nbytes):
    """(buffer, pointer to `nbytes` bytes inside it with 64 KiB of pattern on either side, check)"""
    pad, pattern = 64 * 1024, 0xA5
    buf = torch.full((pad + nbytes + pad,), pattern, dtype=torch.uint8, device="cuda")
    return buf, buf.data_ptr() + pad, (lambda: bool((buf[:pad] == pattern).all()) and bool((buf[pad + nbytes:] == pattern).all()))


@pytest.mark.parametrize("mode,x3", MODES)
@pytest.mark.parametrize("name", ["c", "g-b17", "i"])   # (i: the split-K partial sums live in the workspace)
def test_calls_stay_inside_the_workspace_they_asked_for(name, mode, x3):
    case = BY_NAME[name]
    o, u = oracle_case(case), _model(BY_NAME[name], mode, x3)
    lib, cfg, f = u._lib, case.cfg, case.cfg.downscale
    B, H, W, zh, zw = case.B, case.H, case.W, case.H // f, case.W // f
    x, noise = torch.tensor(o["x"]).cuda(), torch.tensor(o["noise"]).cuda()
    z, mean, log_var = (torch.empty(B, cfg.emb_channels, zh, zw, device="cuda") for _ in range(3))
    nb = u.encode_workspace_bytes(B, H, W)
    buf, ws, intact = _canaried(nb)
    args = (u._h, x.data_ptr(), B, H, W, 1.0, noise.data_ptr(), 0, 0, 0, z.data_ptr(), mean.data_ptr(), log_var.data_ptr())
    assert lib.pf_autoenc_encode(*args, ws, nb - 1, _lib.current_stream()) == -1 and "workspace too small" in lib.pf_last_error().decode()
    _lib.check(lib.pf_autoenc_encode(*args, ws, nb, _lib.current_stream()), "pf_autoenc_encode", lib)
    torch.cuda.synchronize()
    assert intact(), "the encoder wrote outside its workspace"
    errs = {"mean": _err(mean, o["mean"]), "log_var": _err(log_var, o["log_var"]), "z": _err(z, o["z"])}

    zin = torch.tensor(o["z32"]).cuda()
    img = torch.empty(B, cfg.out_channels, H, W, device="cuda")
    nb = u.decode_workspace_bytes(B, zh, zw)
    buf, ws, intact = _canaried(nb)
    args = (u._h, zin.data_ptr(), B, zh, zw, 1.0, img.data_ptr())
    assert lib.pf_autoenc_decode(*args, ws, nb - 1, _lib.current_stream()) == -1 and "workspace too small" in lib.pf_last_error().decode()
    _lib.check(lib.pf_autoenc_decode(*args, ws, nb, _lib.current_stream()), "pf_autoenc_decode", lib)
    torch.cuda.synchronize()
    assert intact(), "the decoder wrote outside its workspace"
    errs["dec"] = _err(img, o["dec"])
    assert max(errs.values()) < TOL, errs


@pytest.mark.parametrize("mode,x3", MODES)
def test_encode_with_null_outputs_writes_the_same_bits_into_the_rest(mode, x3):
    case = BY_NAME["b"]
    o, u = oracle_case(case), _model(case, mode, x3)
    lib, cfg, f = u._lib, case.cfg, case.cfg.downscale
    B, H, W = case.B, case.H, case.W
    shape = (B, cfg.emb_channels, H // f, W // f)
    x, noise = torch.tensor(o["x"]).cuda(), torch.tensor(o["noise"]).cuda()
    nb = u.encode_workspace_bytes(B, H, W)
    ws = torch.empty(nb, dtype=torch.uint8, device="cuda")

    def run(want_z, want_mean, want_lv):
        outs = [torch.full(shape, float("nan"), device="cuda") if w else None for w in (want_z, want_mean, want_lv)]
        _lib.check(lib.pf_autoenc_encode(u._h, x.data_ptr(), B, H, W, 1.0, noise.data_ptr(), 0, 0, 0, *(_lib.ptr(t) for t in outs), ws.data_ptr(), nb,
                                         _lib.current_stream()), "pf_autoenc_encode", lib)
        torch.cuda.synchronize()
        return outs

    z, mean, log_var = run(True, True, True)
    assert not bool(torch.isnan(z).any() | torch.isnan(mean).any() | torch.isnan(log_var).any())
    assert torch.equal(run(True, False, False)[0], z)
    assert torch.equal(run(False, False, True)[2], log_var)
    _, m2, lv2 = run(False, True, True)
    assert torch.equal(m2, mean) and torch.equal(lv2, log_var)
    # none at all: nothing to compute, refused
    assert lib.pf_autoenc_encode(u._h, x.data_ptr(), B, H, W, 1.0, noise.data_ptr(), 0, 0, 0, None, None, None, ws.data_ptr(), nb,
                                 _lib.current_stream()) == -1


def test_shapes_the_plans_cannot_run_are_refused_before_anything_is_launched():
    """Each refusal returns -1 with a message, and leaves the (NaN-filled) outputs untouched.  For the shapes among them the workspace and
    launch queries return 0 first; a zero scale is no shape, the queries know nothing of it."""
    u = _model(BY_NAME["g-b1"], "bf16x3", None)   # the small net: f = 2
    lib = u._lib
    big = 4 * 4 * 68 * 68
    x = torch.randn(big, device="cuda")
    ws = torch.empty(max(u.encode_workspace_bytes(1, 64, 64), u.encode_workspace_bytes(1, 32, 16), u.decode_workspace_bytes(1, 32, 32),
                         u.decode_workspace_bytes(1, 16, 8)), dtype=torch.uint8, device="cuda")
    outs = [torch.full((big,), float("nan"), device="cuda") for _ in range(3)]

    def untouched():
        torch.cuda.synchronize()
        return all(bool(torch.isnan(t).all()) for t in outs)

    def encode(B, H, W):
        return lib.pf_autoenc_encode(u._h, x.data_ptr(), B, H, W, 1.0, None, 0, 0, 0, *(t.data_ptr() for t in outs), ws.data_ptr(), ws.numel(),
                                     _lib.current_stream())

    def decode(B, zh, zw, scale=1.0):
        return lib.pf_autoenc_decode(u._h, x.data_ptr(), B, zh, zw, scale, outs[0].data_ptr(), ws.data_ptr(), ws.numel(), _lib.current_stream())

    # image: a side that is no multiple of 2^(L-1); latents of 10x8 = 80, 32x34 = 1088 tokens; batch 0
    for B, H, W, text in ((1, 33, 16, "image 33x16"), (1, 32, 15, "image 32x15"), (1, 20, 16, "image 20x16"), (1, 64, 68, "image 64x68"),
                          (0, 32, 16, "bad arguments")):
        assert u.encode_workspace_bytes(B, H, W) == 0 and u.encode_launches(B, H, W) == 0 and u.encode_flops(B, H, W) == 0.0
        assert encode(B, H, W) == -1 and text in lib.pf_last_error().decode(), (B, H, W, lib.pf_last_error())
        assert untouched()
    for B, zh, zw, text in ((1, 10, 8, "latent 10x8"), (1, 32, 34, "latent 32x34"), (0, 16, 8, "bad arguments")):
        assert u.decode_workspace_bytes(B, zh, zw) == 0 and u.decode_launches(B, zh, zw) == 0 and u.decode_flops(B, zh, zw) == 0.0
        assert decode(B, zh, zw) == -1 and text in lib.pf_last_error().decode(), (B, zh, zw, lib.pf_last_error())
        assert untouched()
    assert u.decode_workspace_bytes(1, 16, 8) > 0
    assert decode(1, 16, 8, scale=0.0) == -1 and "pf_autoenc_decode: bad arguments" in lib.pf_last_error().decode()
    assert untouched()
    with pytest.raises(RuntimeError, match="does not fit this model"):
        u.encode(torch.zeros(1, 3, 33, 16))
    with pytest.raises(RuntimeError, match="does not fit this model"):
        u.decode(torch.zeros(1, 4, 10, 8))
    # the shapes beside them run
    assert encode(1, 32, 16) == 0 and decode(1, 16, 8) == 0
    assert not untouched()


def test_configurations_the_kernels_cannot_run_are_refused_at_create():
    lib = _lib.load()

    def create(cfg):
        c = _lib.AutoencCfg()
        c.in_channels, c.out_channels, c.channels, c.n_levels = cfg.in_channels, cfg.out_channels, cfg.channels, len(cfg.channel_multipliers)
        for i, m in enumerate(cfg.channel_multipliers):
            c.channel_multipliers[i] = m
        c.n_resnet_blocks, c.z_channels, c.emb_channels = cfg.n_resnet_blocks, cfg.z_channels, cfg.emb_channels
        h = ctypes.c_void_p()
        rc = lib.pf_autoenc_create(ctypes.byref(c), ctypes.byref(h))
        if h:
            lib.pf_autoenc_destroy(h)
        return rc, lib.pf_last_error().decode()

    ok = dict(in_channels=3, out_channels=3, channels=32, channel_multipliers=(1, 2), n_resnet_blocks=1, z_channels=4, emb_channels=4)
    assert create(AutoencoderConfig(**ok))[0] == 0
    for change, text in ((dict(in_channels=5), "in / out channels must be 1..4"),
                         (dict(channels=48), "channels must be a multiple of 32"),
                         # top width 512 with z 4: 512 * 4 * 9 floats = 72 KiB, more than the decoder front's 64 KiB weight stage
                         (dict(channels=128, channel_multipliers=(1, 4)), "decoder conv_in 4 -> 512 does not fit its kernel")):
        rc, msg = create(AutoencoderConfig(**dict(ok, **change)))
        assert rc == -1 and text in msg, (change, rc, msg)
        with pytest.raises(RuntimeError, match="pf_autoenc_create"):
            Autoencoder(AutoencoderConfig(**dict(ok, **change)))
    # ... and 512 with z 3 (54 KiB) fits
    assert create(AutoencoderConfig(**dict(ok, channels=128, channel_multipliers=(1, 4), z_channels=3)))[0] == 0


# ---- pf_gaussian_sample alone ----
SAMPLE_N = (1, 5, 1027)


def _moments(n, seed, first=-30.0):
    """mean, log_var (with both bounds of the clamp among its values; a single element holds `first`) and noise"""
    g = np.random.Generator(np.random.PCG64(seed))
    mean = g.standard_normal(n).astype(np.float32)
    lv = (4.0 * g.standard_normal(n)).astype(np.float32).clip(-30.0, 20.0)
    lv[-1] = 20.0
    lv[0] = first
    noise = g.standard_normal(n).astype(np.float32)
    return mean, lv, noise


@pytest.mark.parametrize("scale", [1.0, 0.18215])
@pytest.mark.parametrize("n", SAMPLE_N)
def test_gaussian_sample_against_float64(n, scale):
    """z = s (m + exp(lv / 2) n) in fp32: the halving is exact, expf is good to 1 ulp, then a product, a sum and a product, each rounded
    once - four roundings of 2^-24 and one of 2^-23 on terms no larger than |s| (|m| + |exp(lv / 2) n|); asserted per element with
    twice that margin and more, 16 * 2^-24.  s is the float32 the call receives."""
    lib = _lib.load()
    seen = set()
    for first in ((-30.0, 20.0) if n == 1 else (-30.0,)):   # one element cannot hold both bounds: two runs
        mean, lv, noise = _moments(n, 100 + n, first)
        seen |= set(lv.tolist())
        m, l, nz = (torch.from_numpy(a).cuda() for a in (mean, lv, noise))
        z = torch.full((n + 8,), float("nan"), device="cuda")
        _lib.check(lib.pf_gaussian_sample(m.data_ptr(), l.data_ptr(), nz.data_ptr(), 0, 0, 0, scale, z.data_ptr(), n, _lib.current_stream()),
                   "pf_gaussian_sample", lib)
        torch.cuda.synchronize()
        assert bool(torch.isnan(z[n:]).all())
        m64, l64, n64 = mean.astype(np.float64), lv.astype(np.float64), noise.astype(np.float64)
        s = float(np.float32(scale))
        sd_n = np.exp(0.5 * l64) * n64
        ref = s * (m64 + sd_n)
        bound = 16.0 * 2.0 ** -24 * abs(s) * (np.abs(m64) + np.abs(sd_n))
        diff = np.abs(z[:n].cpu().numpy().astype(np.float64) - ref)
        print(f"gaussian_sample n={n} scale={scale} log_var[0]={first}: worst diff / bound {float((diff / bound).max()):.3f}")
        assert bool((diff <= bound).all()), float((diff / bound).max())
    assert -30.0 in seen and 20.0 in seen


@pytest.mark.parametrize("offset", [0, 3, 6])
@pytest.mark.parametrize("n", SAMPLE_N)
def test_gaussian_sample_draws_what_randn_writes(n, offset):
    lib = _lib.load()
    seed, stream_id, scale = 21, 4, 0.18215
    mean, lv, _ = _moments(n, 200 + n)
    m, l = torch.from_numpy(mean).cuda(), torch.from_numpy(lv).cuda()
    noise = torch.empty(n, device="cuda")
    _lib.check(lib.pf_randn(noise.data_ptr(), n, seed, stream_id, offset, _lib.current_stream()), "pf_randn", lib)
    z_given, z_rng = torch.empty(n, device="cuda"), torch.empty(n, device="cuda")
    _lib.check(lib.pf_gaussian_sample(m.data_ptr(), l.data_ptr(), noise.data_ptr(), 0, 0, 0, scale, z_given.data_ptr(), n, _lib.current_stream()),
               "pf_gaussian_sample", lib)
    _lib.check(lib.pf_gaussian_sample(m.data_ptr(), l.data_ptr(), None, seed, stream_id, offset, scale, z_rng.data_ptr(), n, _lib.current_stream()),
               "pf_gaussian_sample", lib)
    assert torch.equal(z_rng, z_given)
    assert n < 5 or float(noise.std()) > 0.3   # (the draw is noise, not zeros)
