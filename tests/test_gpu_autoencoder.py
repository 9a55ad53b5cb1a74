"""The first-stage autoencoder on the MI355X against the reference golden (tests/golden/autoencoder.npz, tools/make_goldens_autoencoder.py):
posterior moments, sample, decode and forward of the small net in all three arithmetic modes, the DownSample's padding mode through the
per-op hook, the clamp, the in-kernel noise, the full net inside the workspace its dry walk reports, and LatentDiffusion's two calls.

The contract is the project's standing one: max-abs-diff < 1e-3 against the reference's values (whose rms the fixture generator keeps in
[0.1, 30])."""
import ctypes
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from polyffusion_amd import _lib
from polyffusion_amd.autoencoder import Autoencoder, AutoencoderConfig
from polyffusion_amd.weights import synth_autoencoder_state

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = np.load(os.path.join(REPO, "tests", "golden", "autoencoder.npz"))
SMALL = AutoencoderConfig(in_channels=3, out_channels=3, channels=32, channel_multipliers=(1, 2), n_resnet_blocks=1, z_channels=4,
                          emb_channels=4)
FULL = AutoencoderConfig()
MODES = [("f32", None), ("bf16x3", None), ("f16x3", "f16")]
TOL = 1e-3
_models = {}


def _model(cfg, mode, x3, clamp=False):
    """One handle per (net, library, weights), shared by the tests; the mode is set per use."""
    key = (cfg, x3, clamp)
    if key not in _models:
        st = synth_autoencoder_state(cfg, 0)
        if clamp:   # tools/make_goldens_autoencoder.py clamp_state
            b = st["quant_conv.bias"].copy()
            b[cfg.emb_channels + 0] += np.float32(20.0)
            b[cfg.emb_channels + 1] += np.float32(-30.0)
            st["quant_conv.bias"] = b
        _models[key] = Autoencoder(cfg, x3=x3).load_state_dict(st)
    return _models[key].set_precision(mode)


def _err(got, name):
    e = float((got.detach().cpu().double() - torch.from_numpy(G[name]).double()).abs().max())
    print(f"{name}: max-abs-diff {e:.3e}")
    return e


@pytest.mark.parametrize("mode,x3", MODES)
def test_small_matches_reference(mode, x3):
    u = _model(SMALL, mode, x3)
    x, noise = torch.from_numpy(G["small_x"]).cuda(), torch.from_numpy(G["small_noise"]).cuda()
    post = u.encode(x)
    errs = {"small_mean": _err(post.mean, "small_mean"), "small_log_var": _err(post.log_var, "small_log_var")}
    z = post.sample(noise)
    errs["small_z"] = _err(z, "small_z")
    z_fused, post2 = u.encode_sample(x, noise=noise)
    assert torch.equal(z_fused, z) and torch.equal(post2.mean, post.mean) and torch.equal(post2.log_var, post.log_var)
    # decode on the reference's z (the decoder alone), then the whole forward
    errs["small_dec"] = _err(u.decode(torch.from_numpy(G["small_z"]).cuda()), "small_dec")
    fwd, post3 = u(x, noise=noise)
    errs["small_forward"] = _err(fwd, "small_forward")
    assert torch.equal(post3.mean, post.mean)
    assert fwd.shape == x.shape and z.shape == (3, 4, 16, 8)
    assert max(errs.values()) < TOL, errs


@pytest.mark.parametrize("mode,x3", MODES)
def test_downsample_conv_pads_bottom_and_right_only(mode, x3):
    """F.pad(x, (0, 1, 0, 1)) + Conv2d(3, stride 2, padding 0) alone, on the smallest input with interior, last-row and last-column
    output pixels (6x10 -> 3x5).  Products of O(1) values summed over K = 288: the fp32 / split roundoff is ~1e-6, far inside 1e-3;
    the symmetric padding the same launch computes with pad_mode 0 differs from it by O(1)."""
    lib, B, C, H, W = _lib.load(x3), 3, 32, 6, 10
    g = torch.Generator().manual_seed(6)
    x = torch.randn(B, C, H, W, generator=g)
    w = torch.randn(C, C, 3, 3, generator=g) * (1.0 / (9 * C)) ** 0.5
    bias = torch.randn(C, generator=g) * 0.1
    ref = F.conv2d(F.pad(x.double(), (0, 1, 0, 1)), w.double(), bias.double(), stride=2)
    ref_same = F.conv2d(x.double(), w.double(), bias.double(), stride=2, padding=1)
    assert ref.shape == ref_same.shape == (B, C, 3, 5)
    wp = torch.zeros(lib.pf_packed_gemm_weight_floats(C, C, 9))
    pack = lib.pf_pack_gemm_weight if mode == "f32" else lib.pf_pack_gemm_weight_bf16x3
    _lib.check(pack(w.contiguous().data_ptr(), C, C, 9, wp.data_ptr()), "pack", lib)
    xh, wd, bd = x.permute(0, 2, 3, 1).contiguous().cuda(), wp.cuda(), bias.cuda()

    def run(pad_mode):
        out = torch.full((B, 3, 5, C), float("nan"), device="cuda")
        a = _lib.ConvArgs()
        a.x0, a.c0, a.batch, a.hin, a.win, a.ks, a.stride, a.pad_mode = xh.data_ptr(), C, B, H, W, 3, 2, pad_mode
        a.w, a.n, a.bias, a.out, a.ld_out, a.precision = wd.data_ptr(), C, bd.data_ptr(), out.data_ptr(), C, 0 if mode == "f32" else 1
        info = _lib.ConvPlanInfo()   # a strided conv runs the direct form of its precision, 4x16-pixel x 64-channel tiles
        _lib.check(lib.pf_conv_describe(ctypes.byref(a), ctypes.byref(info)), "pf_conv_describe", lib)
        assert (_lib.CONV_FORMS[info.form], info.tile_h, info.tile_w, info.tile_n) == ("f32" if mode == "f32" else "split", 4, 16, 64)
        _lib.check(lib.pf_conv2d(ctypes.byref(a), _lib.current_stream()), "pf_conv2d", lib)
        torch.cuda.synchronize()
        return out.cpu().permute(0, 3, 1, 2).double()

    e_br, e_same = float((run(_lib.PAD_BOTTOM_RIGHT) - ref).abs().max()), float((run(_lib.PAD_SAME) - ref_same).abs().max())
    print(f"pad bottom/right: {e_br:.3e}; symmetric: {e_same:.3e}")
    assert e_br < TOL and e_same < TOL
    assert float((ref - ref_same).abs().max()) > 0.1
    # an odd side has no such DownSample: refused, not mis-padded
    a = _lib.ConvArgs()
    a.x0, a.c0, a.batch, a.hin, a.win, a.ks, a.stride, a.pad_mode = xh.data_ptr(), C, B, 5, 10, 3, 2, _lib.PAD_BOTTOM_RIGHT
    a.w, a.n, a.out, a.ld_out = wd.data_ptr(), C, xh.data_ptr(), C
    assert lib.pf_conv2d(ctypes.byref(a), _lib.current_stream()) == -1


@pytest.mark.parametrize("mode,x3", MODES)
def test_clamp_sits_exactly_on_the_bounds(mode, x3):
    u = _model(SMALL, mode, x3, clamp=True)
    post = u.encode(torch.from_numpy(G["small_x"]).cuda())
    assert _err(post.mean, "clamp_mean") < TOL and _err(post.log_var, "clamp_log_var") < TOL
    ref = torch.from_numpy(G["clamp_log_var"])
    lv = post.log_var.cpu()
    lo, hi = ref == -30.0, ref == 20.0
    assert int(lo.sum()) >= ref.numel() // 100 and int(hi.sum()) >= ref.numel() // 100
    assert bool((lv[lo] == -30.0).all()) and bool((lv[hi] == 20.0).all())
    assert float(lv.min()) >= -30.0 and float(lv.max()) <= 20.0
    assert torch.allclose(post.std.cpu(), torch.exp(0.5 * ref), rtol=1e-4, atol=0.0)


def test_in_kernel_noise_is_bit_identical_to_randn_and_runs_reproduce():
    u = _model(SMALL, "bf16x3", None)
    lib = u._lib
    x = torch.from_numpy(G["small_x"]).cuda()
    seed, stream_id, offset = 5, 3, 8
    noise = torch.empty(3, 4, 16, 8, device="cuda")
    _lib.check(lib.pf_randn(noise.data_ptr(), noise.numel(), seed, stream_id, offset, _lib.current_stream()), "pf_randn", lib)
    z_rng, post = u.encode_sample(x, seed=seed, stream_id=stream_id, offset=offset)
    z_exp, _ = u.encode_sample(x, noise=noise)
    assert torch.equal(z_rng, z_exp)
    assert torch.equal(post.sample(seed=seed, stream_id=stream_id, offset=offset), z_exp) and torch.equal(post.sample(noise), z_exp)
    assert not torch.equal(u.encode_sample(x, seed=seed + 1, stream_id=stream_id, offset=offset)[0], z_exp)
    # an offset that is no multiple of four starts inside a Philox group
    _lib.check(lib.pf_randn(noise.data_ptr(), noise.numel(), seed, stream_id, 6, _lib.current_stream()), "pf_randn", lib)
    assert torch.equal(u.encode_sample(x, seed=seed, stream_id=stream_id, offset=6)[0], u.encode_sample(x, noise=noise)[0])
    # two calls, same bits
    z2, post2 = u.encode_sample(x, noise=noise)
    z1, post1 = u.encode_sample(x, noise=noise)
    assert torch.equal(z1, z2) and torch.equal(post1.mean, post2.mean) and torch.equal(post1.log_var, post2.log_var)
    assert torch.equal(u.decode(z1), u.decode(z1.clone()))


def _canaried(nbytes):
    """(buffer, pointer to `nbytes` bytes inside it with 64 KiB of pattern on either side)"""
    pad, pattern = 64 * 1024, 0xA5
    buf = torch.full((pad + nbytes + pad,), pattern, dtype=torch.uint8, device="cuda")
    return buf, buf.data_ptr() + pad, (lambda: bool((buf[:pad] == pattern).all()) and bool((buf[pad + nbytes:] == pattern).all()))


@pytest.mark.parametrize("mode,x3", [("f32", None), ("bf16x3", None)])
def test_full_matches_reference_inside_the_workspace_it_asked_for(mode, x3):
    u = _model(FULL, mode, x3)
    lib = u._lib
    x = torch.from_numpy(np.random.Generator(np.random.PCG64(int(G["full_x_seed"]))).standard_normal((1, 3, 128, 128)).astype(np.float32)).cuda()
    mean, log_var = torch.empty(1, 4, 16, 16, device="cuda"), torch.empty(1, 4, 16, 16, device="cuda")
    nb = u.encode_workspace_bytes(1, 128, 128)
    buf, ws, intact = _canaried(nb)
    args = (u._h, x.data_ptr(), 1, 128, 128, 1.0, None, 0, 0, 0, None, mean.data_ptr(), log_var.data_ptr())
    assert lib.pf_autoenc_encode(*args, ws, nb - 1, _lib.current_stream()) == -1 and "workspace too small" in lib.pf_last_error().decode()
    _lib.check(lib.pf_autoenc_encode(*args, ws, nb, _lib.current_stream()), "pf_autoenc_encode", lib)
    torch.cuda.synchronize()
    assert intact(), "the encoder wrote outside its workspace"
    errs = {"full_mean": _err(mean, "full_mean"), "full_log_var": _err(log_var, "full_log_var")}

    z = torch.from_numpy(G["full_mean"]).cuda()
    img = torch.empty(1, 3, 128, 128, device="cuda")
    nb = u.decode_workspace_bytes(1, 16, 16)
    buf, ws, intact = _canaried(nb)
    args = (u._h, z.data_ptr(), 1, 16, 16, 1.0, img.data_ptr())
    assert lib.pf_autoenc_decode(*args, ws, nb - 1, _lib.current_stream()) == -1 and "workspace too small" in lib.pf_last_error().decode()
    _lib.check(lib.pf_autoenc_decode(*args, ws, nb, _lib.current_stream()), "pf_autoenc_decode", lib)
    torch.cuda.synchronize()
    assert intact(), "the decoder wrote outside its workspace"
    errs["full_dec"] = _err(img, "full_dec")
    assert max(errs.values()) < TOL, errs
    assert torch.equal(u.decode(z), img) and torch.equal(u.encode(x).mean, mean)


def test_latent_diffusion_calls_the_autoencoder_with_its_scaling_factor():
    """autoencoder_decode(autoencoder_encode(x)) through LatentDiffusion equals decode(encode(x).sample()) on the handle, bit for bit,
    with the same noise.  The handle is given the same factor: s * z / s is not the identity in fp32 (for s = 0.18215 it moves a
    fraction of the values by one ulp), so the unscaled composition would differ in the last bits whatever the implementation; that
    composition is held to the numerical contract instead."""
    from polyffusion_amd.unet import LatentDiffusion, UNetModel
    u = _model(SMALL, "bf16x3", None)
    unet = UNetModel(in_channels=2, out_channels=2, channels=64, n_res_blocks=1, attention_levels=[1], channel_multipliers=[1, 2], n_heads=4,
                     tf_layers=1, d_cond=128, img_h=32, img_w=32)   # (never evaluated here)
    ldm = LatentDiffusion(unet, u, latent_scaling_factor=0.18215)
    s = ldm.latent_scaling_factor
    x, noise = torch.from_numpy(G["small_x"]).cuda(), torch.from_numpy(G["small_noise"]).cuda()
    z = ldm.autoencoder_encode(x, noise=noise)
    assert torch.equal(z, u.encode(x, scale=s).sample(noise))
    assert float((z.cpu().double() - s * torch.from_numpy(G["small_z"]).double()).abs().max()) < TOL * s
    img = ldm.autoencoder_decode(z)
    assert torch.equal(img, u.decode(u.encode(x, scale=s).sample(noise), scale=s))
    plain = u.decode(u.encode(x).sample(noise))
    assert float((img - plain).abs().max()) < TOL and _err(img, "small_forward") < TOL
    # the Philox path goes through as well
    assert torch.equal(ldm.autoencoder_encode(x, seed=9, stream_id=1), u.encode(x, scale=s).sample(seed=9, stream_id=1))
