"""The training objective, forward only, on the MI355X (-m gpu): pf_qsample_rows and pf_mse_rows against float64 and against their own
other forms (tensor noise / noise drawn in the kernel, whole batch / split batch), then LatentDiffusion.loss, DenoiseDiffusion.loss,
get_loss_dict and validation_loss against what the real reference computed (tests/golden/loss.npz, tools/make_goldens_loss.py)."""
import json
import math
import os
import random
import subprocess
import sys

import numpy as np
import pytest
import torch

from polyffusion_amd import _lib, _steps
from polyffusion_amd.arch import UNetConfig
from polyffusion_amd.ddpm import DDPMConfig, DDPMUNet, DenoiseDiffusion, Polyffusion_DDPM
from polyffusion_amd.model_sdf import Polyffusion_SDF
from polyffusion_amd.unet import LatentDiffusion, UNetModel
from polyffusion_amd.validate import validation_loss
from polyffusion_amd.weights import synth_ddpm_state, synth_unet_state

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = np.load(os.path.join(REPO, "tests", "golden", "loss.npz"))
N_STEPS = 1000
SEED, DRAW, OFF = 11, 3, 8
# rows, row_elems, t: a row far smaller than a workgroup; no multiple of any tile (4108 = 2 * 2048 + 12); the small nets' row
SHAPES = [(3, 20, [0, 999, 999]), (5, 4108, [0, 999, 417, 417, 3]), (4, 2 * 32 * 32, [0, 999, 542, 542])]
SMALL = UNetConfig(in_channels=2, out_channels=2, channels=32, n_res_blocks=1, attention_levels=(1,), channel_multipliers=(1, 2), n_heads=2,
                   tf_layers=1, d_cond=32)
SMALL4 = UNetConfig(in_channels=4, out_channels=2, channels=32, n_res_blocks=1, attention_levels=(1,), channel_multipliers=(1, 2), n_heads=2,
                    tf_layers=1, d_cond=32)
DSMALL = DDPMConfig(image_channels=2, n_channels=32, ch_mults=(1, 2), is_attn=(False, True), n_blocks=2, img_h=32, img_w=32)
MODES = [("f32", None), ("bf16x3", None), ("f16x3", "f16")]


@pytest.fixture(scope="module")
def lib():
    _lib.require_gpu()
    return _lib.load()


@pytest.fixture(scope="module")
def tabs():
    """The float32 tables of the sdf schedule, on the host (float64 copies for the references) and on the device."""
    sa, sb = _steps.sqrt_tables(LatentDiffusion(None).alpha_bar, "cpu")
    return sa, sb, sa.cuda(), sb.cuda()


def gauss(shape, seed, scale=1.0):
    return torch.from_numpy((scale * np.random.Generator(np.random.PCG64(seed)).standard_normal(shape)).astype(np.float32))


def xt_bound(a, b, x0, noise):
    """1.5 * 2^-23 * (|a x0| + |b noise|): three float32 roundings, with or without FMA contraction."""
    return 1.5 * 2.0 ** -23 * ((a * x0.double()).abs() + (b * noise.double()).abs())


# ---- pf_qsample_rows ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,n,t", SHAPES)
def test_qsample_rows(lib, tabs, rows, n, t):
    sa, sb, sa_d, sb_d = tabs
    x0 = gauss((rows, n), 1, 0.5)
    t_h = torch.tensor(t)
    t_d, x0_d = t_h.cuda(), x0.cuda()
    noise_d = _steps.randn(lib, (rows, n), "cuda", SEED, DRAW, OFF)
    noise = noise_d.cpu()
    # tensor form against float64
    got = _steps.qsample_rows(lib, x0_d, t_d, sa_d, sb_d, noise=noise_d)
    a, b = sa[t_h].double()[:, None], sb[t_h].double()[:, None]
    ref = a * x0.double() + b * noise.double()
    err = (got.cpu().double() - ref).abs()
    print(f"qsample rows={rows} n={n}: max err {err.max():.3e}, max err / bound {(err / xt_bound(a, b, x0, noise).clamp_min(1e-300)).max():.3f}")
    assert bool((err <= xt_bound(a, b, x0, noise)).all())
    # noise drawn in the kernel: bit-identical to pf_randn + the tensor form; noise_out is pf_randn
    nz_out = torch.full((rows, n), float("nan"), device="cuda")
    got_rng = _steps.qsample_rows(lib, x0_d, t_d, sa_d, sb_d, rng=(SEED, DRAW, OFF), noise_out=nz_out)
    assert torch.equal(got_rng, got) and torch.equal(nz_out, noise_d)
    assert torch.equal(_steps.qsample_rows(lib, x0_d, t_d, sa_d, sb_d, rng=(SEED, DRAW, OFF)), got)
    # the batch split after two rows, the second part's elem_offset advanced by the rows in front
    parts = [_steps.qsample_rows(lib, x0_d[:2], t_d[:2], sa_d, sb_d, rng=(SEED, DRAW, OFF)),
             _steps.qsample_rows(lib, x0_d[2:], t_d[2:], sa_d, sb_d, rng=(SEED, DRAW, OFF + 2 * n))]
    assert torch.equal(torch.cat(parts), got)


def test_qsample_rows_clamps_a_bad_row_and_refuses_bad_arguments(lib, tabs):
    _, _, sa_d, sb_d = tabs
    x0, nz = gauss((2, 8), 2).cuda(), gauss((2, 8), 3).cuda()
    got = _steps.qsample_rows(lib, x0, torch.tensor([-5, 4000]).cuda(), sa_d, sb_d, noise=nz)
    assert torch.equal(got, _steps.qsample_rows(lib, x0, torch.tensor([0, N_STEPS - 1]).cuda(), sa_d, sb_d, noise=nz))
    t = torch.tensor([1, 2]).cuda()
    with pytest.raises(RuntimeError, match="multiples of 4"):
        _steps.qsample_rows(lib, x0, t, sa_d, sb_d, rng=(0, 0, 2))
    with pytest.raises(RuntimeError, match="noise tensor"):
        _steps.qsample_rows(lib, x0, t, sa_d, sb_d)
    # a row length that is no multiple of 4 takes the element-by-element path of the tensor form
    x5, n5 = gauss((3, 5), 4).cuda(), gauss((3, 5), 5).cuda()
    got = _steps.qsample_rows(lib, x5, torch.tensor([0, 999, 7]).cuda(), sa_d, sb_d, noise=n5)
    ref = _steps.qsample_rows(lib, torch.nn.functional.pad(x5, (0, 3)), torch.tensor([0, 999, 7]).cuda(), sa_d, sb_d,
                              noise=torch.nn.functional.pad(n5, (0, 3)))[:, :5]
    assert torch.equal(got, ref)


# ---- pf_mse_rows -------------------------------------------------------------------------------------------------------------------
def spiked(rows, n, noise):
    """eps_theta = noise - d with |d| ~ 1e-3, except 1e3 times that on each row's last element and around every chunk boundary (and the
    first 16-byte group's edge): a dropped tail or a dropped chunk edge changes the sum by orders of magnitude."""
    d = gauss((rows, n), 7, 1e-3)
    for i in {n - 1, 3, 4} | {c + j for c in range(_lib.MSE_CHUNK, n, _lib.MSE_CHUNK) for j in (-1, 0)}:
        if 0 <= i < n:
            d[:, i] = torch.where(d[:, i] >= 0, 1.0, -1.0) * (1.0 + 0.1 * i / n)
    return noise - d


@pytest.mark.parametrize("rows,n,t", SHAPES)
def test_mse_rows(lib, rows, n, t):
    noise_d = _steps.randn(lib, (rows, n), "cuda", SEED, DRAW, OFF)
    eps_d = spiked(rows, n, noise_d.cpu()).cuda()
    got = _steps.mse_rows(lib, eps_d, noise=noise_d)
    assert got.dtype == torch.float64 and got.shape == (rows,)
    ref = ((noise_d.cpu().double() - eps_d.cpu().double()) ** 2).sum(dim=1)
    rel = ((got.cpu() - ref).abs() / ref).max().item()
    print(f"mse rows={rows} n={n}: max relative error {rel:.3e} (bound {2.0 ** -22:.3e}); row sums {ref.tolist()}")
    assert float(ref.min()) > 2.0       # the spikes dominate: each is worth >= 1
    assert rel <= 2.0 ** -22
    assert torch.equal(_steps.mse_rows(lib, eps_d, noise=noise_d), got)                       # call to call
    assert torch.equal(_steps.mse_rows(lib, eps_d, rng=(SEED, DRAW, OFF)), got)               # noise re-drawn in the kernel
    for kw0, kw1 in ((dict(noise=noise_d[:2]), dict(noise=noise_d[2:])), (dict(rng=(SEED, DRAW, OFF)), dict(rng=(SEED, DRAW, OFF + 2 * n)))):
        parts = [_steps.mse_rows(lib, eps_d[:2], **kw0), _steps.mse_rows(lib, eps_d[2:], **kw1)]
        assert torch.equal(torch.cat(parts), got)                                              # split after two rows
    # rows of zeros: exactly 0 (a row equal to its noise, and all-zero tensors)
    eps_d[1] = noise_d[1]
    z = _steps.mse_rows(lib, eps_d, noise=noise_d)
    assert z[1].item() == 0.0 and torch.equal(z[0], got[0]) and torch.equal(z[2:], got[2:])
    zeros = torch.zeros(rows, n, device="cuda")
    assert torch.equal(_steps.mse_rows(lib, zeros, noise=zeros), torch.zeros(rows, dtype=torch.float64, device="cuda"))


def test_mse_rows_unaligned_row_length_gives_the_bits_of_the_padded_row(lib):
    """A row length that is no multiple of 4 takes the element-by-element loads; the order of the sum is that of the 16-byte form."""
    noise, eps = gauss((3, 2051), 8), gauss((3, 2051), 9)
    got = _steps.mse_rows(lib, eps.cuda(), noise=noise.cuda())
    ref = ((noise.double() - eps.double()) ** 2).sum(dim=1)
    assert ((got.cpu() - ref).abs() / ref).max().item() <= 2.0 ** -22
    pad = lambda v: torch.nn.functional.pad(v, (0, 1)).cuda()
    assert torch.equal(_steps.mse_rows(lib, pad(eps), noise=pad(noise)), got)
    with pytest.raises(RuntimeError, match="multiples of 4"):
        _steps.mse_rows(lib, eps.cuda(), rng=(0, 0, 0))


# ---- end to end on the small nets, against the reference's recorded evaluation --------------------------------------------------------
def sdf_model(mode, x3, cfg=SMALL, hw=32):
    m = UNetModel(in_channels=cfg.in_channels, out_channels=cfg.out_channels, channels=cfg.channels, n_res_blocks=cfg.n_res_blocks,
                  attention_levels=cfg.attention_levels, channel_multipliers=cfg.channel_multipliers, n_heads=cfg.n_heads,
                  tf_layers=cfg.tf_layers, d_cond=cfg.d_cond, img_h=hw, img_w=hw, x3=x3)
    m.load_state_dict(synth_unet_state(cfg, 0))
    m.set_precision(mode)
    return LatentDiffusion(m)


def ddpm_model(mode, x3):
    u = DDPMUNet(DSMALL, x3=x3)
    u.load_state_dict(synth_ddpm_state(DSMALL, 0))
    u.set_precision(mode)
    return DenoiseDiffusion(u, N_STEPS)


def loss_bound(l_ref, delta):
    """|L - L_ref| <= 2 delta sqrt(L_ref) + delta^2 + 2^-20 L_ref: Cauchy-Schwarz on an eps_theta that is within delta of the reference's,
    elementwise, plus the float32 roundings of the reference's own mean."""
    return 2 * delta * math.sqrt(l_ref) + delta * delta + 2.0 ** -20 * l_ref


def sdf_delta(mode):
    return 1e-4 if mode == "f32" else 5e-4     # tests/test_gpu_unet.py (TOL) / tests/test_gpu_bf16x3.py on unet_small.npz


def ddpm_delta(mode, eps_ref):
    # tests/test_gpu_ddpm.py test_unet_small_matches_reference: 1e-3 absolute, and 1e-4 of the output scale in f32
    return min(1e-3, 1e-4 * float(np.abs(eps_ref).max())) if mode == "f32" else 1e-3


def check_xt(got, net, alpha_bar):
    sa, sb = _steps.sqrt_tables(alpha_bar, "cpu")
    t = torch.from_numpy(G[f"{net}_t"])
    x0, noise = torch.from_numpy(G[f"{net}_x0"]), torch.from_numpy(G[f"{net}_noise"])
    a, b = sa[t].double()[:, None, None, None], sb[t].double()[:, None, None, None]
    err = (got.cpu().double() - torch.from_numpy(G[f"{net}_x_t"]).double()).abs()
    print(f"{net} x_t vs the reference's: max |diff| {err.max():.3e}")
    assert bool((err <= xt_bound(a, b, x0, noise)).all())


@pytest.mark.parametrize("mode,x3", MODES)
def test_latent_diffusion_loss_matches_reference(mode, x3):
    ldm = sdf_model(mode, x3)
    x0, cond, noise, t = (torch.from_numpy(G[f"sdf_{k}"]).cuda() for k in ("x0", "cond", "noise", "t"))
    check_xt(ldm.q_sample(x0, t, eps=noise), "sdf", ldm.alpha_bar)
    loss = ldm.loss(x0, cond, noise=noise, t=t)
    rows = ldm.loss_rows(x0, cond, noise=noise, t=t)
    l_ref = float(G["sdf_loss"])
    print(f"sdf {mode}: loss {loss.item():.8f} reference {l_ref:.8f} |diff| {abs(loss.item() - l_ref):.3e} bound {loss_bound(l_ref, sdf_delta(mode)):.3e}")
    assert loss.dim() == 0 and loss.dtype == torch.float32 and rows.dtype == torch.float64 and rows.shape == (4,)
    assert abs(loss.item() - l_ref) <= loss_bound(l_ref, sdf_delta(mode))
    assert torch.equal(loss, rows.mean().float())
    # per sample, against the recorded eps_theta of the reference
    rows_ref = ((G["sdf_noise"].astype(np.float64) - G["sdf_eps_theta"]) ** 2).reshape(4, -1).mean(axis=1)
    for got, ref in zip(rows.cpu().tolist(), rows_ref):
        assert abs(got - ref) <= loss_bound(ref, sdf_delta(mode))


@pytest.mark.parametrize("mode,x3", MODES)
def test_denoise_diffusion_loss_matches_reference(mode, x3):
    d = ddpm_model(mode, x3)
    x0, noise, t = (torch.from_numpy(G[f"ddpm_{k}"]).cuda() for k in ("x0", "noise", "t"))
    check_xt(d.q_sample(x0, t, eps=noise), "ddpm", d.alpha_bar)
    loss = d.loss(x0, noise=noise, t=t)
    rows = d.loss_rows(x0, noise=noise, t=t)
    l_ref, delta = float(G["ddpm_loss"]), ddpm_delta(mode, G["ddpm_eps_theta"])
    print(f"ddpm {mode}: loss {loss.item():.8f} reference {l_ref:.8f} |diff| {abs(loss.item() - l_ref):.3e} bound {loss_bound(l_ref, delta):.3e}")
    assert loss.dim() == 0 and loss.dtype == torch.float32
    assert abs(loss.item() - l_ref) <= loss_bound(l_ref, delta)
    assert torch.equal(loss, rows.mean().float())
    assert torch.equal(Polyffusion_DDPM(d).get_loss_dict((x0, None, None, None), 0, noise=noise, t=t)["loss"], loss)


def test_library_noise_is_the_tensor_noise_and_t_is_checked():
    """noise=None: the noise drawn in the two kernels is pf_randn's - the loss equals, bit for bit, the loss on that tensor; a batch split
    in two sees the noise of the whole batch; t=None is reproducible; a bad t held on the host is refused."""
    ldm = sdf_model("bf16x3", None)
    lib = ldm.eps_model._lib
    x0, cond = torch.from_numpy(G["sdf_x0"]).cuda(), torch.from_numpy(G["sdf_cond"]).cuda()
    t = torch.from_numpy(G["sdf_t"])
    noise = _steps.randn(lib, x0.shape, "cuda", 5, 2, 16)
    rows = ldm.loss_rows(x0, cond, t=t, seed=5, draw=2, elem_offset=16)
    assert torch.equal(rows, ldm.loss_rows(x0, cond, noise=noise, t=t))
    n = x0[0].numel()
    split = torch.cat([ldm.loss_rows(x0[:1], cond[:1], t=t[:1], seed=5, draw=2, elem_offset=16),
                       ldm.loss_rows(x0[1:], cond[1:], t=t[1:], seed=5, draw=2, elem_offset=16 + n)])
    # the UNet's tiles do not depend on the batch size at this shape; should that change, the rows still agree to the net's tolerance
    assert float((split - rows).abs().max()) <= loss_bound(float(rows.max()), 5e-4)
    assert torch.equal(ldm.loss(x0, cond, seed=9), ldm.loss(x0, cond, seed=9))
    rows9, t9 = ldm.loss_rows(x0, cond, seed=9, return_t=True)
    assert torch.equal(t9.cpu(), _steps.time_steps(None, 4, N_STEPS, 9, "cpu")) and bool(torch.isfinite(rows9).all())
    with pytest.raises(RuntimeError, match="outside"):
        ldm.loss(x0, cond, t=[0, 1, 2, N_STEPS])
    d = ddpm_model("bf16x3", None)
    xd = torch.from_numpy(G["ddpm_x0"]).cuda()
    assert torch.equal(d.loss_rows(xd, t=t, seed=5, draw=2, elem_offset=16), d.loss_rows(xd, noise=noise, t=t))
    # DenoiseDiffusion.q_sample with a tensor t: the owner's next draw, made in the kernel
    d.seed, d._draws = 5, 2
    assert torch.equal(d.q_sample(xd, t.cuda()), d.q_sample(xd, t.cuda(), eps=_steps.randn(lib, xd.shape, "cuda", 5, 2, 0))) and d._draws == 3


@pytest.mark.parametrize("mode,x3", MODES)
def test_get_loss_dict_reproduces_the_recorded_cond_modes(mode, x3):
    ldm = sdf_model(mode, x3)
    x0, noise, chord = (torch.from_numpy(G[k]).cuda() for k in ("sdf_x0", "sdf_noise", "gld_chord"))
    batch = (x0, None, chord, torch.zeros(4, 128, 128, device="cuda"))
    for i, (cond_mode, seed) in enumerate(zip(G["gld_modes"], G["gld_seeds"])):
        model = Polyffusion_SDF(ldm, "chord", cond_mode=str(cond_mode))
        random.seed(int(seed))
        out = model.get_loss_dict(batch, 0, noise=noise, t=torch.from_numpy(G["gld_t"][i]))
        l_ref = float(G["gld_loss"][i])
        print(f"get_loss_dict[{cond_mode}, seed {seed}] {mode}: {out['loss'].item():.8f} reference {l_ref:.8f}")
        assert set(out) == {"loss"} and abs(out["loss"].item() - l_ref) <= loss_bound(l_ref, sdf_delta(mode))
    # dropping the condition is visible in the loss: the kept and the dropped mix evaluation differ by far more than the bound
    assert abs(float(G["gld_loss"][2]) - float(G["gld_loss"][3])) > 4 * loss_bound(float(G["gld_loss"][3]), 5e-4)


def small_batches():
    for k, B in enumerate((3, 2)):
        x0 = (gauss((B, 2, 32, 32), 40 + k) > 1.0).float().cuda()
        chord = (gauss((B, 8, 4), 50 + k) > 0.5).float().cuda()
        yield (x0, None, chord, torch.zeros(B, 128, 128, device="cuda"))


@pytest.mark.parametrize("net", ["sdf", "ddpm"])
def test_validation_loss_is_the_mean_of_its_batches_and_buckets_partition_the_samples(net):
    if net == "sdf":
        ldm = sdf_model("bf16x3", None)
        model = Polyffusion_SDF(ldm, "chord")
        one = lambda b, **kw: ldm.loss(b[0], b[2].reshape(-1, 1, 32), **kw)
    else:
        d = ddpm_model("bf16x3", None)
        model = Polyffusion_DDPM(d)
        one = lambda b, **kw: d.loss(b[0], **kw)
    r = validation_loss(model, small_batches(), 2, seed=5)
    assert r["n_samples"] == 5 and r["n_batches"] == 2 and r["t"].shape == r["loss"].shape == (5,)
    losses, lo = [], 0
    for k, b in enumerate(small_batches()):
        B = b[0].shape[0]
        losses.append(float(one(b, t=torch.from_numpy(r["t"][lo:lo + B]), seed=5, draw=k, elem_offset=lo * 2 * 32 * 32)))
        assert math.isclose(losses[-1], r["loss"][lo:lo + B].mean(), rel_tol=1e-6)      # the batch loss is the mean of its rows
        lo += B
    assert r["batch_losses"] == losses and r["val/loss"] == float(np.mean(losses))
    gen = torch.Generator().manual_seed(5)
    assert r["t"].tolist() == torch.randint(0, N_STEPS, (3,), generator=gen).tolist() + torch.randint(0, N_STEPS, (2,), generator=gen).tolist()
    bk = r["t_buckets"]
    assert len(bk) == 10 and bk[0]["t_lo"] == 0 and bk[-1]["t_hi"] == N_STEPS and all(a["t_hi"] == b["t_lo"] for a, b in zip(bk, bk[1:]))
    assert sum(b["count"] for b in bk) == 5
    for b in bk:
        inside = (r["t"] >= b["t_lo"]) & (r["t"] < b["t_hi"])
        assert b["count"] == int(inside.sum())
        assert (b["loss"] is None) if b["count"] == 0 else math.isclose(b["loss"], r["loss"][inside].mean(), rel_tol=1e-12)
    # a second run is the same run
    assert validation_loss(model, small_batches(), None, seed=5)["batch_losses"] == losses


def test_validation_loss_raises_on_a_non_finite_loss():
    class Broken:
        ddpm = type("D", (), {"n_steps": N_STEPS})

        def get_loss_dict(self, batch, step, **kw):
            return {"loss": torch.tensor(float("nan")), "loss_rows": torch.zeros(1, dtype=torch.float64), "t": torch.zeros(1, dtype=torch.int64)}

    with pytest.raises(RuntimeError, match="non-finite"):
        validation_loss(Broken(), [(torch.zeros(1, 2, 4, 4),)], 1)


def test_cond_concat_loss_is_the_loss_of_the_explicit_forward():
    """concat_blurry: loss(..., cond_concat=) == the loss put together from q_sample, forward(cat([x_t, blurry], 1), t, cond) and
    pf_mse_rows, bit for bit (latent_diffusion.py:229-232); and get_loss_dict with concat_blurry takes that road."""
    from polyffusion_amd.inference_sdf import get_blurry_image
    ldm = sdf_model("bf16x3", None, SMALL4, 16)
    lib = ldm.eps_model._lib
    x0 = (gauss((3, 2, 16, 16), 60) > 1.0).float().cuda()
    cond, noise, t = gauss((3, 1, 32), 61).cuda(), gauss((3, 2, 16, 16), 62).cuda(), torch.tensor([0, 999, 417])
    cc = get_blurry_image(x0.clone(), 0.25)
    loss = ldm.loss(x0, cond, noise=noise, cond_concat=cc, t=t)
    xt = ldm.q_sample(x0, t, eps=noise)
    eps = ldm.eps_model(torch.cat([xt, cc], dim=1), t.cuda(), cond)
    want = (_steps.mse_rows(lib, eps, noise=noise) / float(2 * 16 * 16)).mean().float()
    assert torch.equal(loss, want) and math.isfinite(loss.item())
    model = Polyffusion_SDF(ldm, "chord", concat_blurry=True, concat_ratio=0.25)
    chord = cond.reshape(3, 8, 4)
    assert torch.equal(model.get_loss_dict((x0, None, chord, None), 0, noise=noise, t=t)["loss"], loss)


def test_cli_prints_one_json_line_with_a_finite_loss():
    """python -m polyffusion_amd.validate as a fresh process: synthetic weights (sdf_chd8bar), one synthetic batch of 16."""
    env = dict(os.environ, PYTHONPATH=REPO + os.pathsep + os.environ.get("PYTHONPATH", ""))
    p = subprocess.run([sys.executable, "-m", "polyffusion_amd.validate", "--synthetic", "--synthetic_weights", "--batch_num", "1"],
                       cwd=REPO, env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]
    r = json.loads(lines[0])
    assert r["model"] == "sdf_chd8bar" and r["n_samples"] == 16 and r["n_batches"] == 1 and math.isfinite(r["val/loss"]) and r["val/loss"] > 0
    assert sum(b["count"] for b in r["t_buckets"]) == 16
